#!/usr/bin/env python
"""What the skip connection (residual=True) and RMSNorm (norm="rms") cost in the batch-tiled trainer (csrc/mlp_tile.hip),
on one GPU.

  A  (--against TREE)  tools/bench_norm.py's part A: the plain step of this tree against another build of the project
     (the parent commit, built in TREE), `bench.py` in its own process, the trees alternating.  Requirement: this tree's
     median lies inside (or above) the parent's own min .. max in every run.
  B  on this build, in one process: persistent train launches (FusedMLPKernel.prepare_train on the tile plan) of STEPS
     Adam steps with ReLU and dropout 0.2 at B = 256 for 5-64-64-2 and 5-128-128-2: plain, norm="layer", residual,
     norm="rms", residual + rms - the same data, linear parameters and state reset before every window.  The parent's
     plain and LayerNorm steps of the same shapes come from `--parent-shapes` run in the parent's tree with its own
     tools/bench_norm.py protocol: this file's part B restricted to what the parent knows (plain, norm="layer").

tools/bench_optim.py's protocol: every configuration is built and warmed first; then ROUNDS rounds, each timing every
configuration once (alternating, so drift hits all alike): a host clock around work that ends in a device synchronise.
Reported: the median and the min .. max of the rounds, us per step.  The tool fails without a GPU.

    python tools/bench_res.py [--rounds 9] [--parent-shapes] [--against TREE [--bench-rounds 5]] [--label TEXT] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

from bench_accum import part_a  # noqa: E402

MODELS = ([5, 64, 64, 2], [5, 128, 128, 2])
BATCH, STEPS = 256, 500
KINDS = (("plain", {}), ("norm layer", dict(norm="layer")), ("residual", dict(residual=True)),
         ("norm rms", dict(norm="rms")), ("residual + rms", dict(norm="rms", residual=True)))


def tile_configs(dims, dev, kinds):
    import torch

    from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params

    g = torch.Generator().manual_seed(0)
    n = BATCH * STEPS
    lin = (torch.rand(mlp_num_params(dims), generator=g) * 2 - 1) * 0.3
    X = torch.randn(n, dims[0], generator=g).to(dev)
    Y = (torch.rand(n, generator=g) < 0.2).to(torch.int32).to(dev)
    idx = torch.randperm(n, generator=g).to(torch.int32).to(dev)
    out = []
    for label, kw in kinds:
        tail = {None: [], "layer": [t for h in dims[1:-1] for t in (torch.ones(h), torch.zeros(h))],
                "rms": [torch.ones(h) for h in dims[1:-1]]}[kw.get("norm")]
        p0 = torch.cat([lin] + tail).to(dev)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        loss = torch.zeros(STEPS, device=dev)
        bound = FusedMLPKernel(dims, bmax=1024).prepare_train(
            p, m, v, X, Y, idx, n_items=n, batch=BATCH, lr=0.01, dropout=0.2, loss_out=loss, step_counter=counter, **kw)

        def reset(p=p, m=m, v=v, counter=counter, p0=p0):
            p.copy_(p0), m.zero_(), v.zero_(), counter.zero_()

        out.append(("B %s B = %d tile step, %s" % ("-".join(map(str, dims)), BATCH, label), reset,
                    lambda bound=bound: bound.run(0, STEPS), loss))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent-shapes", action="store_true", help="part B with plain and norm=\"layer\" alone")
    ap.add_argument("--bench-rounds", type=int, default=5, help="part A: bench.py runs per tree and model")
    ap.add_argument("--against", default="", help="part A: a tree holding another build of the project (the parent)")
    ap.add_argument("--label", default="", help="printed with the results (which tree this is)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    import torch

    import dct_amd  # noqa: F401

    if not torch.cuda.is_available():
        raise SystemExit("bench_res.py needs a GPU")
    dev = torch.device("cuda", 0)
    lines = ["bench_res %s: %s, %d alternating rounds" % (a.label, torch.cuda.get_device_name(0), a.rounds)]
    built = [c for dims in MODELS for c in tile_configs(dims, dev, KINDS[:2] if a.parent_shapes else KINDS)]
    for name, reset, run, loss in built:
        for _ in range(2):  # warm-up: code objects, workspaces, every shape of the timed window
            reset()
            run()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(loss).all()):
            raise SystemExit("bench_res: non-finite losses in %s" % name)
    times = {c[0]: [] for c in built}
    for _ in range(a.rounds):
        for name, reset, run, _ in built:
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / STEPS * 1e6)
    out = {}
    lines.append("  B: us per step (median, min .. max), %d steps per timed window" % STEPS)
    for name, t in times.items():
        lines.append("  %-60s %9.2f  (%.2f .. %.2f)" % (name, statistics.median(t), min(t), max(t)))
        out[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
    slower = part_a(os.path.abspath(a.against), a.bench_rounds, lines, out) if a.against else []
    lines.append(json.dumps({"label": a.label, "rounds": a.rounds, "results": out}))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if slower:  # the one requirement: the plain step must not pay for the feature
        raise SystemExit("bench_res: this tree's median is below the parent's min .. max in: " + "; ".join(slower))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What AdamW and SGD cost in the batch-tiled trainer (csrc/mlp_tile.hip, MlpArgs::opt_kind), on one GPU.

  A  (--against TREE)  plain Adam of this tree against another build of the project (the parent commit, built in
     TREE): tools/bench_accum.py's part A - `bench.py --batch 256 --steps 2000` for 5-64-2 and 5-128-128-2 and the
     flagship run (3x128 at batch 4, 20,000 steps), one process per run, the trees alternating.  Requirement: this
     tree's median lies inside (or above) the parent's own min .. max in every run; the tool writes its report and then
     exits with an error naming the runs where it lies below.  --only-a skips the rest.
  B  on this build, in one process: persistent train launches (FusedMLPKernel.prepare_train on the tile plan) of STEPS
     steps with Adam, AdamW (wd 0.05) and SGD (momentum 0.9), for 5-64-2 and 5-128-128-2 at B = 256 and B = 32 - the
     same data, parameters and state reset before every window.  The optimizer lives in the fold kernel alone; SGD
     loads and stores p and m only and has no division.
  C  the reference-config model (5-64-2, batch 4) with SGD (momentum 0.9): the fused engine on the tile plan against
     the autograd engine with torch.optim.SGD, which such a model took before the fold knew SGD.

B / C: every configuration is built and warmed first; then ROUNDS rounds, each timing every configuration once
(alternating, so drift hits all alike): a host clock around work that ends in a device synchronise.  Reported: the
median and the min .. max of the rounds, us per step.  The tool fails without a GPU.

    python tools/bench_optim.py [--rounds 9] [--against TREE [--bench-rounds 5] [--only-a]] [--label TEXT] [--out FILE]
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

from bench_accum import part_a  # noqa: E402  (the plain step against the parent: the same runs, the same rule)

MODELS = ([5, 64, 2], [5, 128, 128, 2])
BATCHES, STEPS = (256, 32), 500
OPTIMIZERS = (("Adam", {}), ("AdamW wd 0.05", dict(optimizer="adamw", weight_decay=0.05)),
              ("SGD momentum 0.9", dict(optimizer="sgd", momentum=0.9)))


def tile_configs(dims, dev):
    import torch

    from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params

    g = torch.Generator().manual_seed(0)
    n = max(BATCHES) * STEPS
    p0 = ((torch.rand(mlp_num_params(dims), generator=g) * 2 - 1) * 0.3).to(dev)
    X = torch.randn(n, dims[0], generator=g).to(dev)
    Y = (torch.rand(n, generator=g) < 0.2).to(torch.int32).to(dev)
    idx = torch.randperm(n, generator=g).to(torch.int32).to(dev)
    name = "-".join(map(str, dims))
    out = []
    for b in BATCHES:
        for label, kw in OPTIMIZERS:
            kern = FusedMLPKernel(dims, bmax=1024)
            p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
            counter = torch.zeros(1, dtype=torch.int32, device=dev)
            loss = torch.zeros(STEPS, device=dev)
            bound = kern.prepare_train(p, m, v, X, Y, idx, n_items=b * STEPS, batch=b, lr=0.01, loss_out=loss,
                                       step_counter=counter, **kw)

            def reset(p=p, m=m, v=v, counter=counter):
                p.copy_(p0), m.zero_(), v.zero_(), counter.zero_()

            out.append(("B %s B = %3d tile step, %s" % (name, b, label), reset,
                        lambda bound=bound: bound.run(0, STEPS), STEPS, loss))
    return out


def engine_configs(dev):
    import torch

    from dct_amd.data.synthetic import weather_tensors
    from dct_amd.models.mlp import MLPClassifier
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import AutogradEngine, FusedMLPEngine, optim_hparams_of

    steps, b = 500, 4
    rows = steps * b + 64
    x, y = weather_tensors(rows, seed=0)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(42))
    ctx = init_distributed("gpu")
    out = []

    def model():
        torch.manual_seed(0)
        return MLPClassifier(5, (64,), dropout=0.2, optimizer="sgd", momentum=0.9)

    fm = model()
    feng = FusedMLPEngine(fm, ctx, b, seed=42, adam=optim_hparams_of(fm.configure_optimizers()))
    assert feng.kind == "sgd" and feng.kernel.plan.trainer(b, optimizer="sgd") == "tile"
    feng.attach_data(x, y, perm[: steps * b], perm[steps * b:])
    n_f = feng.upload_epoch_indices(0)
    floss = torch.zeros(steps, device=dev)
    out.append(("C 5-64-2 batch %d SGD momentum 0.9, fused engine (tile trainer)" % b, lambda: None,
                lambda: feng.run_steps(n_f, steps, floss), steps, floss))
    am = model()
    aeng = AutogradEngine(am, ctx, b, seed=42)
    assert aeng.torch_optimizer is not None  # torch.optim.SGD itself
    aeng.attach_data(x, y, perm[: steps * b], perm[steps * b:])
    arows = aeng.train_rows[aeng.epoch_local_indices(len(aeng.train_rows), 0, True)].to(dev)
    aloss = torch.zeros(steps, device=dev)
    out.append(("C 5-64-2 batch %d SGD momentum 0.9, autograd engine (torch.optim.SGD)" % b, lambda: None,
                lambda: aeng.run_device_steps(arows, 0, steps, aloss), steps, aloss))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--bench-rounds", type=int, default=5, help="part A: bench.py runs per tree and model")
    ap.add_argument("--against", default="", help="part A: a tree holding another build of the project (the parent)")
    ap.add_argument("--only-a", action="store_true", help="part A alone (with --against)")
    ap.add_argument("--label", default="", help="printed with the results (which tree this is)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    import torch

    import dct_amd  # noqa: F401

    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs a GPU")
    dev = torch.device("cuda", 0)
    lines = ["bench_optim %s: %s, %d alternating rounds" % (a.label, torch.cuda.get_device_name(0), a.rounds)]
    out = {}
    built = [] if a.only_a else [c for dims in MODELS for c in tile_configs(dims, dev)] + engine_configs(dev)
    for name, reset, run, steps, loss in built:
        for _ in range(2):  # warm-up: code objects, workspaces, every shape of the timed window
            reset()
            run()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(loss).all()):
            raise SystemExit("bench_optim: non-finite losses in %s" % name)
    times = {c[0]: [] for c in built}
    for _ in range(a.rounds):
        for name, reset, run, steps, _ in built:
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e6)
    lines.append("  B / C: us per step (median, min .. max), steps per timed window in brackets")
    for name, _, _, steps, _ in built:
        t = times[name]
        lines.append("  %-76s %9.2f  (%.2f .. %.2f)  [%d]" % (name, statistics.median(t), min(t), max(t), steps))
        out[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
    slower = part_a(os.path.abspath(a.against), a.bench_rounds, lines, out) if a.against else []
    lines.append(json.dumps({"label": a.label, "rounds": a.rounds, "results": out}))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if slower:  # the one requirement: plain Adam must not pay for the feature
        raise SystemExit("bench_optim: this tree's Adam median is below the parent's min .. max in: " + "; ".join(slower))


if __name__ == "__main__":
    main()

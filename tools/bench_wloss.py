#!/usr/bin/env python
"""What class weights / label smoothing cost in the batch-tiled trainer (csrc/mlp_tile.hip), on one GPU.

  A  (--against TREE)  the unweighted tile step of this tree against another build of the project (the parent
     commit, built in TREE): `bench.py --model M --batch 256 --steps 2000` for 5-64-2 and 5-128-128-2, and the
     flagship `bench.py` run (3x128 at batch 4, 20,000 steps), one process per run, the two trees alternating;
     samples/s per run, the median and the min .. max of each tree.
  B  weighted against unweighted on this build, in one process: persistent train launches of 2000 steps at batch 256
     (FusedMLPKernel.prepare_train on the tile plan), the same data, parameters reset before every window.
  C  the weighted reference-config job's step (MLPClassifier(5, (64,), class_weight, label_smoothing), batch 4): the
     fused engine on the tile plan against the autograd engine, both through their own step loops.

B and C: every configuration is built and warmed first; then ROUNDS rounds, each timing every configuration once
(alternating, so drift hits all alike): a host clock around work that ends in a device synchronise.  Reported: the
median and the min .. max of the rounds, us per step.  The tool fails without a GPU; it sets no threshold.

    python tools/bench_wloss.py [--rounds 9] [--against TREE [--bench-rounds 5]] [--label TEXT] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (bench.py model, name, batch, steps, warm-up): the two tile-trainer runs, and the flagship (mlp_block5, batch 4),
# whose kernels take the same MlpArgs
BENCH_RUNS = (("weather", "5-64-2", 256, 2000, 200), ("weather-mlp-3x128", "5-128-128-2", 256, 2000, 200),
              ("weather-mlp-3x128", "5-128-128-2", 4, 20000, 2000))
MODELS = ([5, 64, 2], [5, 128, 128, 2])
B, STEPS = 256, 2000


def bench_py(tree, model, batch, steps, warmup):
    """samples/s of one `bench.py` run in ``tree`` (its own process)."""
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--model", model, "--batch",
                        str(batch), "--steps", str(steps), "--warmup", str(warmup)], capture_output=True, text=True,
                       cwd=tree, timeout=300)
    if r.returncode != 0:
        raise SystemExit("bench_wloss: bench.py failed in %s:\n%s" % (tree, r.stderr[-2000:]))
    return float(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"])


def part_a(parent, rounds, lines, out):
    for model, name, batch, steps, warmup in BENCH_RUNS:
        vals = {"parent": [], "this": []}
        for r in range(rounds):
            vals["parent"].append(bench_py(parent, model, batch, steps, warmup))
            vals["this"].append(bench_py(ROOT, model, batch, steps, warmup))
            print("  A %s batch %d round %d: parent %.0f this %.0f samples/s"
                  % (name, batch, r, vals["parent"][-1], vals["this"][-1]), flush=True)
        for who in ("parent", "this"):
            v = vals[who]
            lines.append("  A %-12s batch %3d unweighted, bench.py --steps %d, %-6s %10.0f samples/s  (%.0f .. %.0f)  "
                         "runs: %s" % (name, batch, steps, who, statistics.median(v), min(v), max(v),
                                       " ".join("%.0f" % x for x in v)))
        out["A %s batch %d" % (name, batch)] = vals


def tile_configs(dims, dev):
    import torch

    from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params

    g = torch.Generator().manual_seed(0)
    n = B * STEPS
    p0 = ((torch.rand(mlp_num_params(dims), generator=g) * 2 - 1) * 0.3).to(dev)
    X = torch.randn(n, dims[0], generator=g).to(dev)
    Y = (torch.rand(n, generator=g) < 0.2).to(torch.int32).to(dev)  # a minority class
    idx = torch.randperm(n, generator=g).to(torch.int32).to(dev)
    w = torch.tensor([1.0, 3.0], device=dev)
    name = "-".join(map(str, dims))
    out = []
    for what, kw in (("unweighted", {}), ("weights + smoothing", dict(class_weight=w, label_smoothing=0.1)),
                     ("smoothing only", dict(label_smoothing=0.1))):
        kern = FusedMLPKernel(dims, bmax=1024)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        loss = torch.zeros(STEPS, device=dev)
        bound = kern.prepare_train(p, m, v, X, Y, idx, n_items=n, batch=B, lr=0.01, loss_out=loss,
                                   step_counter=counter, **kw)

        def reset(p=p, m=m, v=v, counter=counter):
            p.copy_(p0), m.zero_(), v.zero_(), counter.zero_()

        def run(bound=bound):
            bound.run(0, STEPS)

        out.append(("B %s batch %d tile trainer, %s" % (name, B, what), reset, run, STEPS, loss))
    return out


def engine_configs(dev):
    import torch

    from dct_amd.data.synthetic import weather_tensors
    from dct_amd.models.mlp import MLPClassifier
    from dct_amd.parallel.dist import init_distributed
    from dct_amd.trainer.engines import AutogradEngine, FusedMLPEngine, adam_hparams_from

    steps, b = 2000, 4
    rows = steps * b + 64
    x, y = weather_tensors(rows, seed=0)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(42))
    ctx = init_distributed("gpu")
    out = []

    def model():
        torch.manual_seed(0)
        return MLPClassifier(5, (64,), class_weight=[1.0, 3.0], label_smoothing=0.1, dropout=0.0)

    fm = model()
    feng = FusedMLPEngine(fm, ctx, b, seed=42, adam=adam_hparams_from(fm.configure_optimizers()))
    assert feng.weighted and feng.kernel.plan.trainer(b, weighted=True) == "tile"
    feng.attach_data(x, y, perm[: steps * b], perm[steps * b:])
    n_f = feng.upload_epoch_indices(0)
    floss = torch.zeros(steps, device=dev)
    out.append(("C 5-64-2 batch %d weighted, fused engine (tile trainer)" % b, lambda: None,
                lambda: feng.run_steps(n_f, steps, floss), steps, floss))
    am = model()
    aeng = AutogradEngine(am, ctx, b, seed=42)
    aeng.attach_data(x, y, perm[: steps * b], perm[steps * b:])
    arows = aeng.train_rows[aeng.epoch_local_indices(len(aeng.train_rows), 0, True)].to(dev)
    aloss = torch.zeros(steps, device=dev)
    out.append(("C 5-64-2 batch %d weighted, autograd engine" % b, lambda: None,
                lambda: aeng.run_device_steps(arows, 0, steps, aloss), steps, aloss))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--bench-rounds", type=int, default=5, help="part A: bench.py runs per tree and model")
    ap.add_argument("--against", default="", help="part A: a tree holding another build of the project (the parent)")
    ap.add_argument("--label", default="", help="printed with the results (which tree this is)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    import torch

    import dct_amd  # noqa: F401

    if not torch.cuda.is_available():
        raise SystemExit("bench_wloss.py needs a GPU")
    dev = torch.device("cuda", 0)
    lines = ["bench_wloss %s: %s, %d alternating rounds" % (a.label, torch.cuda.get_device_name(0), a.rounds)]
    out = {}
    built = [c for dims in MODELS for c in tile_configs(dims, dev)] + engine_configs(dev)
    for name, reset, run, steps, loss in built:
        for _ in range(2):  # warm-up: code objects, workspaces, graph capture, every shape of the timed window
            reset()
            run()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(loss).all()):
            raise SystemExit("bench_wloss: non-finite losses in %s" % name)
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
        lines.append("  %-64s %9.2f  (%.2f .. %.2f)  [%d]" % (name, statistics.median(t), min(t), max(t), steps))
        out[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
    if a.against:
        part_a(os.path.abspath(a.against), a.bench_rounds, lines, out)
    lines.append(json.dumps({"label": a.label, "rounds": a.rounds, "results": out}))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

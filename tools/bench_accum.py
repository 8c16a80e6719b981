#!/usr/bin/env python
"""What accumulate_grad_batches costs and buys in the batch-tiled trainer (csrc/mlp_tile.hip), on one GPU.

  A  (--against TREE)  the plain (K = 1) step of this tree against another build of the project (the parent commit,
     built in TREE): `bench.py --model M --batch 256 --steps 2000` for 5-64-2 and 5-128-128-2, and the flagship
     `bench.py` run (3x128 at batch 4, 20,000 steps), one process per run, the two trees alternating (and which of
     them goes first alternating too); samples/s per run, the median and the min .. max of each tree.  --only-a
     skips part B.
  B  on this build, in one process, at B = 256 and B = 32 and K = 2, 4, 8: persistent train launches
     (FusedMLPKernel.prepare_train on the tile plan) of STEPS optimizer steps, the same data, parameters reset before
     every window -
       the accumulated step: one grid of K * ceil(B / 32) workgroups and one fold;
       K plain steps of B rows (K launch pairs), reported per K steps;
       where K * B <= 1024, one plain step of K * B rows (the same rows in one batch).

B: every configuration is built and warmed first; then ROUNDS rounds, each timing every configuration once
(alternating, so drift hits all alike): a host clock around work that ends in a device synchronise.  Reported: the
median and the min .. max of the rounds, us per optimizer step; part B sets no threshold.  Part A's requirement: this
tree's median lies inside (or above) the parent's own min .. max in every run - the tool writes its report and then
exits with an error naming the runs where it lies below.  The tool fails without a GPU.

    python tools/bench_accum.py [--rounds 9] [--against TREE [--bench-rounds 5] [--only-a]] [--label TEXT] [--out FILE]
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
BATCHES, KS, STEPS = (256, 32), (2, 4, 8), 500


def bench_py(tree, model, batch, steps, warmup):
    """samples/s of one `bench.py` run in ``tree`` (its own process)."""
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--model", model, "--batch",
                        str(batch), "--steps", str(steps), "--warmup", str(warmup)], capture_output=True, text=True,
                       cwd=tree, timeout=300)
    if r.returncode != 0:
        raise SystemExit("bench_accum: bench.py failed in %s:\n%s" % (tree, r.stderr[-2000:]))
    return float(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"])


def part_a(parent, rounds, lines, out):
    """Returns the runs in which this tree's median lies below the parent's own min .. max (the requirement)."""
    slower = []
    for model, name, batch, steps, warmup in BENCH_RUNS:
        vals = {"parent": [], "this": []}
        for r in range(rounds):
            # the tree that goes first alternates too: the second process of a pair starts on a device the first one
            # has just left
            for who in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
                vals[who].append(bench_py(parent if who == "parent" else ROOT, model, batch, steps, warmup))
            print("  A %s batch %d round %d: parent %.0f this %.0f samples/s"
                  % (name, batch, r, vals["parent"][-1], vals["this"][-1]), flush=True)
        for who in ("parent", "this"):
            v = vals[who]
            lines.append("  A %-12s batch %3d K = 1, bench.py --steps %d, %-6s %10.0f samples/s  (%.0f .. %.0f)  "
                         "runs: %s" % (name, batch, steps, who, statistics.median(v), min(v), max(v),
                                       " ".join("%.0f" % x for x in v)))
        med = statistics.median(vals["this"])
        where = "inside" if min(vals["parent"]) <= med <= max(vals["parent"]) else (
            "ABOVE" if med > max(vals["parent"]) else "BELOW")
        lines.append("  A %-12s batch %3d: this tree's median %s the parent's min .. max" % (name, batch, where))
        out["A %s batch %d" % (name, batch)] = vals
        if where == "BELOW":
            slower.append("%s batch %d" % (name, batch))
    return slower


def tile_configs(dims, dev):
    import torch

    from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params

    g = torch.Generator().manual_seed(0)
    n = max(BATCHES) * max(KS) * STEPS
    p0 = ((torch.rand(mlp_num_params(dims), generator=g) * 2 - 1) * 0.3).to(dev)
    X = torch.randn(n, dims[0], generator=g).to(dev)
    Y = (torch.rand(n, generator=g) < 0.2).to(torch.int32).to(dev)
    idx = torch.randperm(n, generator=g).to(torch.int32).to(dev)
    name = "-".join(map(str, dims))
    out = []

    def config(what, batch, steps, per, **kw):
        """A persistent launch of ``steps`` steps of ``batch`` rows; reported per ``per`` of them."""
        kern = FusedMLPKernel(dims, bmax=1024)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        loss = torch.zeros(steps, device=dev)
        rows = batch * kw.get("accumulate", 1) * steps
        bound = kern.prepare_train(p, m, v, X, Y, idx, n_items=rows, batch=batch, lr=0.01, loss_out=loss,
                                   step_counter=counter, **kw)

        def reset():
            p.copy_(p0), m.zero_(), v.zero_(), counter.zero_()

        out.append(("B %s %s" % (name, what), reset, lambda: bound.run(0, steps), steps // per, loss))

    for b in BATCHES:
        for k in KS:
            config("B = %3d K = %d: accumulated step (one grid of %d workgroups)" % (b, k, k * -(-b // 32)), b, STEPS,
                   1, accumulate=k)
            config("B = %3d K = %d: %d plain steps of %d rows" % (b, k, k, b), b, STEPS * k, k)
            if k * b <= 1024:
                config("B = %3d K = %d: one plain step of %d rows" % (b, k, k * b), k * b, STEPS, 1)
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
        raise SystemExit("bench_accum.py needs a GPU")
    dev = torch.device("cuda", 0)
    lines = ["bench_accum %s: %s, %d alternating rounds" % (a.label, torch.cuda.get_device_name(0), a.rounds)]
    out = {}
    built = [] if a.only_a else [c for dims in MODELS for c in tile_configs(dims, dev)]
    for name, reset, run, steps, loss in built:
        for _ in range(2):  # warm-up: code objects, workspaces, every shape of the timed window
            reset()
            run()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(loss).all()):
            raise SystemExit("bench_accum: non-finite losses in %s" % name)
    times = {c[0]: [] for c in built}
    for _ in range(a.rounds):
        for name, reset, run, steps, _ in built:
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e6)
    lines.append("  B: us per optimizer step of K * B rows (median, min .. max), %d optimizer steps per timed window"
                 % STEPS)
    for name, _, _, steps, _ in built:
        t = times[name]
        lines.append("  %-76s %9.2f  (%.2f .. %.2f)" % (name, statistics.median(t), min(t), max(t)))
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
        raise SystemExit("bench_accum: this tree's K = 1 median is below the parent's min .. max in: " + "; ".join(slower))


if __name__ == "__main__":
    main()

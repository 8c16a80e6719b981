#!/usr/bin/env python
"""Cost of gradient clipping per training step, on one GPU, in one process and one binary.

  TabTransformer (4 layers, 64 feature tokens, d 64; batch 512; AutogradEngine device loop):   clipping off, by norm
  tabular MLP 256-1024-1024-1024-2 (batch 4096; GraphMLPEngine, eager enqueue):                clipping off, by norm,
                                                            and DCT_DW_INTO_ADAM=0 with clipping off (every dW through g,
                                                            one flat Adam: the clipped step without the norm kernel)

Every configuration is built and warmed first; then ROUNDS rounds, each timing every configuration once (alternating,
so drift hits all alike): a host clock around STEPS steps that end in a device synchronise.  Reported per configuration:
the median and the min .. max of the rounds, us per step.  --no-clip leaves the clipped configurations out and never
names the new arguments, so the same file measures a tree from before gradient clipping.

    python tools/bench_clip.py [--rounds 9] [--steps 2000] [--no-clip] [--label TEXT]
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

CHUNK = 400  # steps per run_steps / run_device_steps call


def tt_config(ctx, clip):
    import torch

    from dct_amd.data.synthetic import make_tabular_device
    from dct_amd.models import build_model
    from dct_amd.trainer.engines import AutogradEngine

    B, feats = 512, 64
    rows = B * (CHUNK + 8)
    X, Y = make_tabular_device(rows, feats, num_classes=2, device=ctx.device, dtype=torch.float32, seed=0)
    torch.manual_seed(0)
    model = build_model("tabtransformer", feats, d_model=64, heads=4, layers=4, lr=1e-3)
    eng = AutogradEngine(model, ctx, B, seed=42, **clip)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(42))
    eng.attach_data(X, Y, perm, perm[:B])
    rows_dev = eng.train_rows.to(ctx.device)
    loss = torch.zeros(CHUNK, device=ctx.device)

    def run():
        eng.run_device_steps(rows_dev, 0, CHUNK, loss)

    return run, eng


def tab_config(ctx, clip, dw_into_adam=None):
    import torch

    from dct_amd.data.synthetic import make_tabular_device
    from dct_amd.models.mlp import build_mlp
    from dct_amd.trainer.engines import adam_hparams_from
    from dct_amd.trainer.graph_engine import GraphMLPEngine

    B, feats = 4096, 256
    rows = B * (CHUNK + 8)
    X, Y = make_tabular_device(rows, feats, num_classes=2, device=ctx.device, dtype=torch.bfloat16, seed=0)
    torch.manual_seed(0)
    model = build_mlp("tabular-mlp-4x1024", feats)
    old = os.environ.get("DCT_DW_INTO_ADAM")
    if dw_into_adam is not None:
        os.environ["DCT_DW_INTO_ADAM"] = dw_into_adam  # read when the executor is built
    try:
        eng = GraphMLPEngine(model, ctx, B, seed=42, adam=adam_hparams_from(model.configure_optimizers()), **clip)
    finally:
        if dw_into_adam is not None:
            if old is None:
                del os.environ["DCT_DW_INTO_ADAM"]
            else:
                os.environ["DCT_DW_INTO_ADAM"] = old
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(42))
    eng.attach_data(X, Y, perm, perm[:B])
    n_items = eng.upload_epoch_indices(0)
    loss = torch.zeros(CHUNK + 8, device=ctx.device)

    def run():
        eng.run_steps(n_items, CHUNK, loss)

    return run, eng


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=2000, help="steps per timed window (a multiple of %d)" % CHUNK)
    ap.add_argument("--no-clip", action="store_true", help="only the configurations without clipping")
    ap.add_argument("--label", default="", help="printed with the results (which tree this is)")
    a = ap.parse_args()
    import torch

    import dct_amd  # noqa: F401
    from dct_amd.parallel.dist import init_distributed

    if not torch.cuda.is_available():
        raise SystemExit("bench_clip.py needs a GPU")
    ctx = init_distributed("gpu")
    on = dict(gradient_clip_val=1.0, gradient_clip_algorithm="norm")
    configs = [("tabtransformer b512, clipping off", lambda: tt_config(ctx, {}))]
    if not a.no_clip:
        configs.append(("tabtransformer b512, clip by norm", lambda: tt_config(ctx, on)))
    configs.append(("tabular 4x1024 b4096, clipping off", lambda: tab_config(ctx, {})))
    configs.append(("tabular 4x1024 b4096, clipping off, DCT_DW_INTO_ADAM=0", lambda: tab_config(ctx, {}, "0")))
    if not a.no_clip:
        configs.append(("tabular 4x1024 b4096, clip by norm", lambda: tab_config(ctx, on)))
    calls = max(1, a.steps // CHUNK)
    built = []
    for name, make in configs:
        run, eng = make()
        for _ in range(2):  # warm-up: code objects, graph capture, every shape of the timed window
            run()
        torch.cuda.synchronize()
        built.append((name, run, eng))
    times = {name: [] for name, _, _ in built}
    for _ in range(a.rounds):
        for name, run, _ in built:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / (calls * CHUNK) * 1e6)
    print("bench_clip %s: %s, %d rounds of %d steps, us per step (median, min .. max)"
          % (a.label, torch.cuda.get_device_name(0), a.rounds, calls * CHUNK))
    out = {}
    for name, _, eng in built:
        t = times[name]
        extra = ""
        if hasattr(eng, "grad_clip_stats") and getattr(eng, "clip_val", None) is not None:
            extra = "   last step {norm, coef} = {%.4g, %.4g}" % eng.grad_clip_stats()
        print("  %-58s %8.2f  (%.2f .. %.2f)%s" % (name, statistics.median(t), min(t), max(t), extra))
        out[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
    print(json.dumps({"label": a.label, "rounds": a.rounds, "steps": calls * CHUNK, "us_per_step": out}))


if __name__ == "__main__":
    main()

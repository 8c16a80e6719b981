#!/usr/bin/env python
"""Cost of the device learning-rate table per training step, on one GPU, in one process and one binary.

  mlp_block5 (3x128 weather MLP, batch 4) and the 5-64-2 wave kernel (batch 4): one persistent launch of 20,000
                                              steps, the long-run step time:                 no table, step-interval table
  captured flat-Adam step, 17,730 parameters (one launch per replay: all latency, where the table's dependent load
                                              shows most):                                   no table, step-interval table
  TabTransformer (4 layers, 64 feature tokens, d 64; batch 512; AutogradEngine device loop):  no table, step-interval table
  tabular MLP 256-1024-1024-1024-2 (batch 4096; GraphMLPEngine, Adam riding in the dW launches): no table, table
  host time to fill one epoch's table of 25,000 steps from a SequentialLR(LinearLR warm-up -> CosineAnnealingLR)

Every configuration is built and warmed first; then ROUNDS rounds, each timing every configuration once (alternating,
so drift hits all alike): a host clock around STEPS steps that end in a device synchronise.  Reported per configuration:
the median and the min .. max of the rounds, us per step.  --no-table leaves the table configurations out and never
names the new arguments, so the same file measures a tree from before the table.

    python tools/bench_lr.py [--rounds 9] [--steps 2000] [--no-table] [--label TEXT]
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
FILL_STEPS = 25000


def make_schedule(ctx, steps):
    """An LrSchedule over its own small optimizer: a step-interval warm-up then cosine decay, its table filled for
    ``steps`` steps from step 0 (the timed windows run past it: those steps read the clamped last entry)."""
    import torch
    from torch.optim import lr_scheduler as S

    from dct_amd.trainer.lr_schedule import LrSchedule

    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    warm = S.LinearLR(opt, start_factor=0.1, total_iters=steps // 10)
    cos = S.CosineAnnealingLR(opt, T_max=steps - steps // 10, eta_min=1e-5)
    sched = LrSchedule(opt, S.SequentialLR(opt, [warm, cos], milestones=[steps // 10]), "step")
    t0 = time.perf_counter()
    sched.begin_epoch(0, steps, device=ctx.device)
    return sched, time.perf_counter() - t0


LONG = 20000  # steps of one persistent launch


def persistent_config(dims):
    def make(ctx, table):
        import torch

        from dct_amd.data.synthetic import weather_tensors
        from dct_amd.ops.fused_mlp import FusedMLPKernel, mlp_num_params

        B = 4
        X, Y = weather_tensors(LONG * B, seed=0)
        dev = ctx.device
        gen = torch.Generator().manual_seed(0)
        p = (torch.randn(mlp_num_params(dims), generator=gen) * 0.1).to(dev)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        idx = torch.randperm(LONG * B, generator=gen).to(dev, torch.int32)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        loss = torch.zeros(LONG, device=dev)
        k = FusedMLPKernel(dims, bmax=4)
        kw = dict(lr_tab=make_schedule(ctx, LONG)[0].device_table(dev)) if table else {}
        bound = k.prepare_train(p, m, v, X.to(dev), Y.to(dev, torch.int32), idx, n_items=LONG * B, batch=B, lr=1e-3,
                                dropout=0.2, seed=1, loss_out=loss, step_counter=counter, **kw)

        def run():
            counter.zero_()  # every launch walks the table from its start
            bound.run(0, LONG)

        run.steps = LONG
        return run, k.plan.trainer(B, mode=0, steps=LONG)
    return make


def flat_config(ctx, table):
    import torch

    from dct_amd.ops.optim import FlatAdam

    n = 17730  # the 3x128 weather MLP's parameter count
    gen = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=gen).to(ctx.device)
    g = (torch.randn(n, generator=gen) * 1e-2).to(ctx.device)
    fa = FlatAdam(p, g, [p.shape], lr=1e-3)
    if table:
        fa.lr_schedule = make_schedule(ctx, CHUNK)[0]
    for _ in range(3):
        fa.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(ctx.device)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            fa.step()
    torch.cuda.current_stream().wait_stream(s)

    def run():
        for _ in range(CHUNK):
            graph.replay()

    return run, fa


def tt_config(ctx, table):
    import torch

    from dct_amd.data.synthetic import make_tabular_device
    from dct_amd.models import build_model
    from dct_amd.trainer.engines import AutogradEngine

    B, feats = 512, 64
    rows = B * (CHUNK + 8)
    X, Y = make_tabular_device(rows, feats, num_classes=2, device=ctx.device, dtype=torch.float32, seed=0)
    torch.manual_seed(0)
    model = build_model("tabtransformer", feats, d_model=64, heads=4, layers=4, lr=1e-3)
    eng = AutogradEngine(model, ctx, B, seed=42)
    if table:
        eng.optimizer.lr_schedule = make_schedule(ctx, CHUNK)[0]  # before the step is captured
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(42))
    eng.attach_data(X, Y, perm, perm[:B])
    rows_dev = eng.train_rows.to(ctx.device)
    loss = torch.zeros(CHUNK, device=ctx.device)

    def run():
        eng.run_device_steps(rows_dev, 0, CHUNK, loss)

    return run, eng


def tab_config(ctx, table):
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
    kw = dict(lr_schedule=make_schedule(ctx, CHUNK)[0]) if table else {}
    eng = GraphMLPEngine(model, ctx, B, seed=42, adam=adam_hparams_from(model.configure_optimizers()), **kw)
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
    ap.add_argument("--no-table", action="store_true", help="only the configurations without a rate table")
    ap.add_argument("--label", default="", help="printed with the results (which tree this is)")
    a = ap.parse_args()
    import torch

    import dct_amd  # noqa: F401
    from dct_amd.parallel.dist import init_distributed

    if not torch.cuda.is_available():
        raise SystemExit("bench_lr.py needs a GPU")
    ctx = init_distributed("gpu")
    configs = []
    for name, make in (("mlp_block5 3x128 b4, 20,000-step launch", persistent_config([5, 128, 128, 2])),
                       ("5-64-2 wave kernel b4, 20,000-step launch", persistent_config([5, 64, 2])),
                       ("captured flat Adam, 17,730 parameters", flat_config), ("tabtransformer b512", tt_config),
                       ("tabular 4x1024 b4096", tab_config)):
        configs.append((name + ", no table", lambda make=make: make(ctx, False)))
        if not a.no_table:
            configs.append((name + ", step-interval table", lambda make=make: make(ctx, True)))
    calls = max(1, a.steps // CHUNK)
    built = []
    for name, make in configs:
        run, eng = make()
        for _ in range(2):  # warm-up: code objects, graph capture, every shape of the timed window
            run()
        torch.cuda.synchronize()
        built.append((name, run, eng))
    times = {name: [] for name, _, _ in built}
    fills = []
    for _ in range(a.rounds):
        for name, run, _ in built:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_calls = 1 if hasattr(run, "steps") else calls
            for _ in range(n_calls):
                run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / (n_calls * getattr(run, "steps", CHUNK)) * 1e6)
        if not a.no_table:
            fills.append(make_schedule(ctx, FILL_STEPS)[1] * 1e3)
    print("bench_lr %s: %s, %d rounds of %d steps (persistent launches: 20,000), us per step (median, min .. max)"
          % (a.label, torch.cuda.get_device_name(0), a.rounds, calls * CHUNK))
    out = {}
    for name, _, eng in built:
        t = times[name]
        print("  %-58s %8.2f  (%.2f .. %.2f)" % (name, statistics.median(t), min(t), max(t)))
        out[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
    if fills:
        print("  host fill of one epoch's table, %d steps (scheduler stepped per entry + upload), ms: %8.2f  (%.2f .. %.2f)"
              % (FILL_STEPS, statistics.median(fills), min(fills), max(fills)))
        out["table fill %d steps" % FILL_STEPS] = {"median_ms": statistics.median(fills), "min_ms": min(fills),
                                                   "max_ms": max(fills)}
    print(json.dumps({"label": a.label, "rounds": a.rounds, "steps": calls * CHUNK, "results": out}))


if __name__ == "__main__":
    main()

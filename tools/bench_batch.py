#!/usr/bin/env python
"""Per-rank batch sweep of the weather MLPs: the batch-tiled fused trainer against the autograd engine.

For each model (weather = 5-64-2, weather-mlp-3x128 = 5-128-128-2, both Dropout 0.2) and batch
(17, 64, 256, 1024) it runs ``Trainer.fit`` on 100k synthetic rows for 3 epochs, once with
``engine="fused"`` and once with ``engine="autograd"``, alternating the two three times in this one
process, and prints the last epoch's ``step_time_ms`` / ``samples_per_sec`` as min-max over the
repeats.  The autograd engine is what these workloads ran on before the tile trainer existed.

    python tools/bench_batch.py [--models weather,weather-mlp-3x128] [--batches 17,64,256,1024]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

import dct_amd  # noqa: E402,F401
from dct_amd.data.dataset import TensorPairDataset  # noqa: E402
from dct_amd.data.synthetic import weather_tensors  # noqa: E402
from dct_amd.models.mlp import build_mlp  # noqa: E402
from dct_amd.tracking import InMemoryLogger  # noqa: E402
from dct_amd.trainer import Trainer, seed_everything  # noqa: E402


def one_fit(model_name, batch, engine, ds, epochs):
    seed_everything(42)
    logger = InMemoryLogger()
    tr = Trainer(max_epochs=epochs, accelerator="gpu", engine=engine, logger=logger, num_sanity_val_steps=0,
                 verbose=False)
    tr.fit(build_mlp(model_name, 5), DataLoader(ds, batch_size=batch, shuffle=True))
    assert tr.engine.name == engine, (tr.engine.name, engine)
    return logger.history("step_time_ms")[-1][1], logger.history("samples_per_sec")[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="weather,weather-mlp-3x128")
    ap.add_argument("--batches", default="17,64,256,1024")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    x, y = weather_tensors(a.rows, seed=0, dim=5)
    ds = TensorPairDataset(x, y)
    print(f"{'model':<20}{'batch':>6}  {'engine':<9}{'step_time_ms (min-max)':>26}{'samples/s (min-max)':>28}", flush=True)
    lost = []
    for model_name in a.models.split(","):
        for batch in (int(b) for b in a.batches.split(",")):
            res = {"fused": [], "autograd": []}
            for _ in range(a.repeats):
                for engine in ("fused", "autograd"):
                    res[engine].append(one_fit(model_name, batch, engine, ds, a.epochs))
            for engine in ("fused", "autograd"):
                ms = [r[0] for r in res[engine]]
                sps = [r[1] for r in res[engine]]
                print(f"{model_name:<20}{batch:>6}  {engine:<9}{min(ms):>12.4f} - {max(ms):<11.4f}"
                      f"{min(sps):>14.0f} - {max(sps):<11.0f}", flush=True)
            if min(r[0] for r in res["fused"]) >= min(r[0] for r in res["autograd"]):
                lost.append((model_name, batch))
    print("fused slower than autograd at: " + (", ".join(f"{m} batch {b}" for m, b in lost) or "no point"), flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()

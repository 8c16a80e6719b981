"""Worker for tests/test_accum_ddp_cpu.py: a W-rank gloo DDP fit with Trainer(accumulate_grad_batches=K) on the CPU
(autograd engine, the torch bucket reducer).  Every rank dumps its final flat parameters, its optimizer-step count and
how often its reducer ran an all-reduce round (finalize) and was handed a gradient (mark_ready)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from torch.utils.data import DataLoader, random_split  # noqa: E402

import dct_amd  # noqa: E402,F401
from dct_amd.data.dataset import TensorPairDataset  # noqa: E402
from dct_amd.data.synthetic import weather_tensors  # noqa: E402
from dct_amd.models.mlp import MLPClassifier  # noqa: E402
from dct_amd.parallel.reducer import TorchBucketReducer  # noqa: E402
from dct_amd.trainer import DDPStrategy, Trainer, seed_everything  # noqa: E402


def main():
    out_dir, epochs, rows, K = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    calls = {"finalize": 0, "mark_ready": 0}
    for name in calls:
        orig = getattr(TorchBucketReducer, name)

        def counted(self, *a, _orig=orig, _name=name, **kw):
            calls[_name] += 1
            return _orig(self, *a, **kw)

        setattr(TorchBucketReducer, name, counted)
    seed_everything(42)
    x, y = weather_tensors(rows, seed=0)
    n_tr = int(0.8 * rows)
    tr, va = random_split(TensorPairDataset(x, y), [n_tr, rows - n_tr])
    model = MLPClassifier(5, hidden=(64,), dropout=0.0)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    trainer = Trainer(max_epochs=epochs, accelerator="cpu", num_nodes=world,
                      strategy=DDPStrategy(find_unused_parameters=False), logger=None, log_every_n_steps=5,
                      engine="autograd", verbose=False, num_sanity_val_steps=0, accumulate_grad_batches=K)
    trainer.fit(model, DataLoader(tr, batch_size=4, shuffle=True), DataLoader(va, batch_size=4))
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).tolist()
    rank = int(os.environ.get("RANK", "0"))
    with open(os.path.join(out_dir, f"params_rank{rank}.json"), "w") as f:
        json.dump({"params": flat, "global_step": trainer.global_step, "engine": trainer.engine.name,
                   "reducer": type(trainer.engine.reducer).__name__, "n_params": len(trainer.engine.params),
                   "train_loss": trainer.callback_metrics.get("train_loss"), **calls}, f)


if __name__ == "__main__":
    main()

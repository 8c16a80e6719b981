"""``Trainer.validate`` / ``Trainer.test`` / ``Trainer.predict``: inference over a dataset, outside ``fit``.

Lightning's three evaluation entry points (``trainer.validate(model, loader)``, ``trainer.test(model, loader,
ckpt_path="best")``, ``trainer.predict(model, loader)``) on two paths:

  * native: the batch-tiled inference kernel (csrc/mlp_infer.hip, ``FusedMLPKernel.infer``).  Taken when the device
    is a GPU, the model has ``fused_spec()`` with an architecture ``FusedMLPKernel.infer_supported`` accepts, and the
    step the call would run (``validation_step`` / ``test_step`` / ``predict_step``, and ``forward``) is the library's
    own, not a user override.  The table is uploaded once and ONE launch covers the rank's whole shard;
    ``validate`` / ``test`` read the launch's statistics (fp64 loss sum, integer counts - the same bits whatever the
    grid; a class-weighted / label-smoothed model reports the weighted mean ``sum num_i / sum w[y_i]`` over the
    rank's whole shard), ``predict`` returns views of one ``[n, C]`` logits tensor split by the loader's batch size, and
    ``trainer.last_confusion_matrix`` holds the int64 ``[C, C]`` confusion matrix (rows = label, columns =
    prediction) summed over ranks.
  * generic: every other model (the wide-MLP and TabTransformer engines' models included) and the CPU -
    ``model.eval()``, ``torch.no_grad()`` and the Python step loop of ``Trainer._validate``'s non-epoch-engine branch.
    ``trainer.last_confusion_matrix`` is None.

All three work without a prior ``fit``: they initialise the distributed context themselves, build no training engine
and need no optimizer.  After a ``fit`` in the same process the engine's weights are first copied into the model.
Under DDP ``validate`` / ``test`` shard with ``distributed_indices(..., shuffle=False)`` and report the cross-rank
mean, exactly as ``fit``'s validation does: when the row count is no multiple of the world size, the rows that pad
the shards are counted twice (in the metrics and in the confusion matrix).  ``predict`` returns each rank's own shard.
``trainer.input_norm = (mean, std)`` (fp32 ``[D0]`` tensors, zero std already replaced by 1) makes both paths score
``(x - mean) / std`` in fp32 - the scoring script's ``"raw": true`` contract.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import torch

from ..ckpt.lightning_io import load_checkpoint
from ..data.dataset import dataset_tensors
from ..data.sampler import distributed_indices
from ..ops.fused_mlp import TILE_BMAX, FusedMLPKernel, weighted_infer_stats
from ..parallel.dist import init_distributed

_STEP = {"val": "validation_step", "test": "test_step", "predict": "predict_step"}
_ROOT = __name__.split(".")[0]


def resolve_ckpt_path(trainer, ckpt_path: str) -> str:
    """``"best"`` / ``"last"`` through the trainer's ModelCheckpoint (ValueError without one, or without such a
    path); anything else is a file."""
    if ckpt_path not in ("best", "last"):
        return ckpt_path
    cb = trainer.checkpoint_callback
    if cb is None:
        raise ValueError(f'ckpt_path="{ckpt_path}" needs a ModelCheckpoint callback on the Trainer')
    path = cb.best_model_path if ckpt_path == "best" else cb.last_model_path
    if not path:
        raise ValueError(f'ckpt_path="{ckpt_path}": the ModelCheckpoint callback has saved no such checkpoint')
    return path


def _one_loader(dataloaders, what: str):
    if isinstance(dataloaders, (list, tuple)):
        if len(dataloaders) != 1:
            raise ValueError(f"Trainer.{what} takes one dataloader, got a list of {len(dataloaders)}")
        dataloaders = dataloaders[0]
    if dataloaders is None:
        raise ValueError(f"Trainer.{what} needs a dataloader")
    return dataloaders


def _tensors(ds) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(features, labels or None) of a dataset, a Subset chain, or a bare feature tensor."""
    if isinstance(ds, torch.Tensor):
        return ds, None
    if isinstance(ds, torch.utils.data.TensorDataset) and len(ds.tensors) == 1:
        return ds.tensors[0], None
    X, Y = dataset_tensors(ds)
    return X, Y


def _library_own(model, name: str) -> bool:
    fn = getattr(type(model), name, None)
    return fn is not None and getattr(fn, "__module__", "").split(".")[0] == _ROOT


def native_path(model, device: torch.device, stage: str) -> bool:
    """The three conditions of the native path (module docstring)."""
    if device.type != "cuda" or not hasattr(model, "fused_spec"):
        return False
    if not (_library_own(model, _STEP[stage]) and _library_own(model, "forward")):
        return False
    return FusedMLPKernel.infer_supported(model.fused_spec()["dims"])


def _prepare(trainer, model, dataloaders, ckpt_path, stage: str):
    what = {"val": "validate", "test": "test", "predict": "predict"}[stage]
    model = model if model is not None else getattr(trainer, "_model", None)
    if model is None:
        raise ValueError(f"Trainer.{what} needs a model (none given, and no fit has run)")
    if dataloaders is None and stage == "val":
        dataloaders = getattr(trainer, "_fit_loaders", (None, None))[1]
    loader = _one_loader(dataloaders, what)
    if trainer.ctx is None:
        trainer.ctx = init_distributed(trainer.accelerator, trainer.strategy.backend, trainer.strategy.timeout_s)
    engine = trainer.engine if getattr(trainer.engine, "model", None) is model else None
    if engine is not None:
        engine.sync_to_model()
    if ckpt_path:
        ckpt = load_checkpoint(resolve_ckpt_path(trainer, ckpt_path))
        model.load_state_dict(ckpt["state_dict"])  # weights only: no optimizer state
        if engine is not None:
            engine.load_from_model()
    if trainer.engine is None:
        trainer._model = model  # (a fit's model stays the trainer's: its engine belongs to it)
    object.__setattr__(model, "_trainer", trainer)
    info = trainer._loader_info(loader)
    X, Y = _tensors(info["dataset"])
    return model, X, Y, info["batch_size"]


def _local_rows(trainer, n: int) -> torch.Tensor:
    return distributed_indices(n, trainer.world_size, trainer.global_rank, shuffle=False)


def _norm_on(trainer, device) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    norm = getattr(trainer, "input_norm", None)
    if norm is None:
        return None
    mean, std = (torch.as_tensor(t, dtype=torch.float32).contiguous().to(device) for t in norm)
    return mean, std


def _flat_params(model, device) -> torch.Tensor:
    parts = []
    for lin in model.linear_layers():
        parts += [lin.weight, lin.bias]
    return torch.cat([t.detach().float().reshape(-1).cpu() for t in parts]).to(device)


def _native_launch(trainer, model, X, Y, local, want_logits: bool):
    """One ``infer`` launch over the rank's shard: (logits or None, (loss mean, correct, confusion) or None)."""
    dev = trainer.ctx.device
    spec = model.fused_spec()
    kern = FusedMLPKernel(spec["dims"], bmax=TILE_BMAX)
    C = spec["dims"][-1]
    n = len(local)
    Xd = X.to(dev, torch.float32).contiguous()
    Yd = Y.to(dev, torch.int32).contiguous() if Y is not None else None
    idx = None if trainer.world_size == 1 else local.to(dev, torch.int32)
    logits = torch.empty(n, C, dtype=torch.float32, device=dev) if want_logits else None
    stats = torch.zeros(2 + C * C, dtype=torch.int64, device=dev) if Yd is not None else None
    # a class-weighted / label-smoothed model (models/mlp.py): the launch sums the weighted numerators, and the mean
    # is sum_i num_i / sum_i w[y_i] over the shard
    cw = spec.get("class_weight")
    eps = float(spec.get("label_smoothing", 0.0))
    weighted = Yd is not None and (cw is not None or eps != 0.0)
    wl = {}
    if weighted:
        wl = dict(class_weight=None if cw is None else torch.as_tensor(cw, dtype=torch.float32).contiguous().to(dev),
                  label_smoothing=eps)
    kern.infer(_flat_params(model, dev), Xd, n, idx=idx, Y=Yd, loss=spec["loss"], logits_out=logits,
               stats_out=stats, norm=_norm_on(trainer, dev), **wl)
    if stats is None:
        return logits, None
    loss_sum, correct, conf = kern.infer_stats(stats)
    if weighted:
        return logits, weighted_infer_stats(loss_sum, correct, conf, cw)
    return logits, (loss_sum / max(1, n), correct, conf)


def _batches(trainer, model, X, Y, local, B: int):
    """The generic path's batches on the device, in loader order: (x, y) pairs, or x alone without labels."""
    dev = trainer.ctx.device
    model.to(dev)
    Xd = X.to(dev, torch.float32)
    norm = _norm_on(trainer, dev)
    if norm is not None:
        Xd = (Xd - norm[0]) / norm[1]
    Yd = Y.to(dev, torch.int64) if Y is not None else None
    rows_all = local.to(dev)
    for bi in range(math.ceil(len(local) / B)):
        rows = rows_all[bi * B: (bi + 1) * B]
        yield bi, len(rows), (Xd[rows] if Yd is None else (Xd[rows], Yd[rows]))


@torch.no_grad()
def run_eval(trainer, stage: str, model=None, dataloaders=None, ckpt_path: Optional[str] = None) -> List[Dict[str, float]]:
    """``validate`` (stage "val") / ``test``: one dict of metrics per dataloader (one is supported)."""
    model, X, Y, B = _prepare(trainer, model, dataloaders, ckpt_path, stage)
    if Y is None:
        raise ValueError("the dataloader's dataset has no labels")
    ctx = trainer.ctx
    local = _local_rows(trainer, len(X))
    trainer.last_confusion_matrix = None
    if native_path(model, ctx.device, stage):
        _, (loss_mean, correct, conf) = _native_launch(trainer, model, X, Y, local, want_logits=False)
        n = max(1, len(local))
        vals = ctx.all_reduce_mean(torch.tensor([loss_mean, correct / n], dtype=torch.float64)).tolist()
        conf = conf.to(ctx.device) if ctx.backend == "nccl" else conf
        trainer.last_confusion_matrix = ctx.all_reduce_sum_(conf).cpu()
        out = {f"{stage}_loss": vals[0], f"{stage}_acc": vals[1]}
    else:
        was_training = model.training
        model.eval()
        trainer._stage = stage
        trainer._epoch_logs = {}
        try:
            step = getattr(model, _STEP[stage])
            for bi, nb, batch in _batches(trainer, model, X, Y, local, B):
                trainer._cur_batch_size = nb
                step(batch, bi)
            out = trainer._reduce_epoch_logs()
        finally:
            trainer._stage = "idle"
            model.train(was_training)
    trainer.callback_metrics.update(out)
    if out:
        trainer._log_metrics(out, trainer.global_step)
    return [out]


@torch.no_grad()
def run_predict(trainer, model=None, dataloaders=None, ckpt_path: Optional[str] = None,
                return_predictions: bool = True) -> Optional[List[Any]]:
    """The per-batch ``predict_step`` outputs in loader order (each rank its own shard)."""
    model, X, Y, B = _prepare(trainer, model, dataloaders, ckpt_path, "predict")
    local = _local_rows(trainer, len(X))
    if native_path(model, trainer.ctx.device, "predict"):
        logits, _ = _native_launch(trainer, model, X, None, local, want_logits=True)
        preds = list(torch.split(logits, B))
    else:
        was_training = model.training
        model.eval()
        try:
            preds = [model.predict_step(batch, bi) for bi, _, batch in _batches(trainer, model, X, Y, local, B)]
        finally:
            model.train(was_training)
    return preds if return_predictions else None

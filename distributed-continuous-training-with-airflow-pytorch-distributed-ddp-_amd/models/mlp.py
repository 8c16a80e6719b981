"""MLP model family.

``WeatherClassifier`` is the reference model, layer for layer
(jobs/train_lightning_ddp.py:51-88): ``net = Sequential(Linear(D,64), ReLU, Dropout(0.2),
Linear(64,2))``, cross-entropy, ``save_hyperparameters()`` -> ``{"input_dim": D}``, Adam(lr=0.01).
Its state_dict keys (``net.0.weight`` ... ``net.3.bias``) are the contract consumed by the
deployment ``score.py`` (dags/azure_manual_deploy.py:66-75,109).

``MLPClassifier`` generalises it (depth, widths, dropout, loss in {ce, mse}) and keeps the same
``net.<3*i>`` key scheme, which covers the BASELINE.json configs (3-layer/128-h weather MLP,
4-layer/1024-h x 256-feature tabular MLP).  Both expose ``fused_spec()`` so the trainer can run
them on the fused HIP kernels (small widths) or the bf16 MFMA GEMM path (large widths); the
torch ``forward`` is the CPU path and the numerical reference.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.fused_mlp import check_class_weight, check_label_smoothing, check_optimizer
from ..trainer.module import TrainModule

# configure_optimizers()'s options and their defaults, which reproduce the reference's Adam(lr): a model records only
# the ones that differ (checkpoints, YAML), so a default model records what it always did
OPTIM_DEFAULTS = dict(optimizer="adam", weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False,
                      betas=(0.9, 0.999), eps=1e-8)


class MLPClassifier(TrainModule):
    def __init__(self, input_dim: int, hidden: Sequence[int] = (64,), num_classes: int = 2, dropout: float = 0.2,
                 loss: str = "ce", lr: float = 0.01, class_weight: Optional[Sequence[float]] = None,
                 label_smoothing: float = 0.0, optimizer: str = "adam", weight_decay: float = 0.0,
                 momentum: float = 0.0, nesterov: bool = False, betas: Sequence[float] = (0.9, 0.999),
                 eps: float = 1e-8, dampening: float = 0.0):
        super().__init__()
        self.save_hyperparameters()
        # the optimizer configure_optimizers() builds: torch.optim.Adam / AdamW / SGD, checked with torch's rules here
        # (an unknown name, a negative decay or momentum, Nesterov without momentum or with dampening: ValueError)
        self.optim = dict(optimizer=check_optimizer(optimizer, weight_decay, momentum, dampening, nesterov),
                          weight_decay=float(weight_decay), momentum=float(momentum), dampening=float(dampening),
                          nesterov=bool(nesterov), betas=tuple(float(b) for b in betas), eps=float(eps))
        for key, default in OPTIM_DEFAULTS.items():
            if key in self.hparams:
                if self.optim[key] != default:
                    self.hparams[key] = list(self.optim[key]) if key == "betas" else self.optim[key]
                else:
                    del self.hparams[key]
        if loss not in ("ce", "mse"):
            raise ValueError("loss must be 'ce' or 'mse'")
        # torch's CrossEntropyLoss(weight=, label_smoothing=): exactly num_classes finite, strictly positive weights,
        # smoothing in [0, 1); cross-entropy only
        w = check_class_weight(class_weight, num_classes)
        self.label_smoothing = check_label_smoothing(label_smoothing)
        if loss != "ce" and (w is not None or self.label_smoothing != 0.0):
            raise ValueError("class_weight / label_smoothing apply to loss='ce' only")
        # recorded hyper-parameters: plain Python numbers (checkpoints, YAML), and only when set - a model without
        # the two options records what it always did
        for key, on, val in (("class_weight", w is not None, None if w is None else [float(x) for x in w.tolist()]),
                             ("label_smoothing", self.label_smoothing != 0.0, self.label_smoothing)):
            if key in self.hparams:
                if on:
                    self.hparams[key] = val
                else:
                    del self.hparams[key]
        # a buffer follows .to(device); non-persistent: the state_dict keys stay net.<i>.weight / bias
        self.register_buffer("class_weight", w, persistent=False)
        dims = [int(input_dim)] + [int(h) for h in hidden] + [int(num_classes)]
        layers: List[nn.Module] = []
        for i in range(len(dims) - 1):
            layers.append(nn.Linear(dims[i], dims[i + 1]))
            if i < len(dims) - 2:
                layers += [nn.ReLU(), nn.Dropout(dropout)]
        self.net = nn.Sequential(*layers)
        self.dims = dims
        self.dropout_p = float(dropout)
        self.loss_kind = loss
        self.lr = lr

    def forward(self, x):
        return self.net(x)

    def compute_loss(self, logits, y):
        if self.loss_kind == "ce":
            return F.cross_entropy(logits, y, weight=self.class_weight, label_smoothing=self.label_smoothing)
        return F.mse_loss(logits, F.one_hot(y, logits.shape[-1]).to(logits.dtype))

    def training_step(self, batch, batch_idx):
        x, y = batch
        loss = self.compute_loss(self(x), y)
        self.log("train_loss", loss, sync_dist=True)
        return loss

    def validation_step(self, batch, batch_idx):
        x, y = batch
        logits = self(x)
        loss = self.compute_loss(logits, y)
        acc = (torch.argmax(logits, dim=1) == y).float().mean()
        self.log("val_loss", loss, sync_dist=True, prog_bar=True)
        self.log("val_acc", acc, sync_dist=True, prog_bar=True)
        return loss

    def test_step(self, batch, batch_idx):
        x, y = batch
        logits = self(x)
        loss = self.compute_loss(logits, y)
        acc = (torch.argmax(logits, dim=1) == y).float().mean()
        self.log("test_loss", loss, sync_dist=True, prog_bar=True)
        self.log("test_acc", acc, sync_dist=True, prog_bar=True)
        return loss

    def configure_optimizers(self):
        o = self.optim
        if o["optimizer"] == "sgd":
            return torch.optim.SGD(self.parameters(), lr=self.lr, momentum=o["momentum"], dampening=o["dampening"],
                                   weight_decay=o["weight_decay"], nesterov=o["nesterov"])
        cls = torch.optim.AdamW if o["optimizer"] == "adamw" else torch.optim.Adam
        return cls(self.parameters(), lr=self.lr, betas=o["betas"], eps=o["eps"], weight_decay=o["weight_decay"])

    # ---- fused-engine contract
    def fused_spec(self):
        spec = {"dims": list(self.dims), "dropout": self.dropout_p, "loss": self.loss_kind}
        # only when set: a spec without them is the plain loss every engine and kernel takes
        if self.class_weight is not None:
            spec["class_weight"] = self.class_weight.detach().float().cpu()
        if self.label_smoothing != 0.0:
            spec["label_smoothing"] = self.label_smoothing
        return spec

    def linear_layers(self) -> List[nn.Linear]:
        return [m for m in self.net if isinstance(m, nn.Linear)]


class WeatherClassifier(MLPClassifier):
    """Reference model: Linear(D,64)-ReLU-Dropout(0.2)-Linear(64,2), CE, Adam(lr=0.01)."""

    def __init__(self, input_dim: int, class_weight: Optional[Sequence[float]] = None, label_smoothing: float = 0.0,
                 **optim):
        super().__init__(input_dim=input_dim, hidden=(64,), num_classes=2, dropout=0.2, loss="ce", lr=0.01,
                         class_weight=class_weight, label_smoothing=label_smoothing, **optim)
        # the reference records exactly {"input_dim": D} (save_hyperparameters at :53); the loss and optimizer options
        # join it only when set
        hp = {"input_dim": int(input_dim)}
        hp.update({k: self.hparams[k] for k in OPTIM_DEFAULTS if k in self.hparams})
        if self.class_weight is not None:
            hp["class_weight"] = [float(x) for x in self.class_weight.tolist()]
        if self.label_smoothing != 0.0:
            hp["label_smoothing"] = self.label_smoothing
        self._set_hparams(hp)


def build_mlp(name: str, input_dim: int, hidden: Optional[Sequence[int]] = None, num_classes: int = 2,
              dropout: float = 0.2, loss: str = "ce", lr: float = 0.01,
              class_weight: Optional[Sequence[float]] = None, label_smoothing: float = 0.0,
              **optim) -> MLPClassifier:
    """``optim``: MLPClassifier's optimizer options (OPTIM_DEFAULTS' keys)."""
    if name == "weather":
        return WeatherClassifier(input_dim, class_weight=class_weight, label_smoothing=label_smoothing, **optim)
    # name -> (hidden widths, dropout, loss, lr); BASELINE.json configs 1-4
    presets = {
        "weather-mlp-3x128": ((128, 128), 0.2, "ce", 0.01),
        "tabular-mlp-4x1024": ((1024, 1024, 1024), 0.0, "mse", 1e-3),
    }
    if name in presets and hidden is None:
        hidden, dropout, loss, lr = presets[name]
    return MLPClassifier(input_dim, hidden=hidden or (64,), num_classes=num_classes, dropout=dropout, loss=loss, lr=lr,
                         class_weight=class_weight, label_smoothing=label_smoothing, **optim)

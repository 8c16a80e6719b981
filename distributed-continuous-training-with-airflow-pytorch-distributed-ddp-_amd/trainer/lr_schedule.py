"""Learning-rate schedulers (``configure_optimizers()`` returning ``lr_scheduler``), Lightning 2.1 semantics.

The step engines take the learning rate as a launch argument of kernels that are captured into graphs, so a rate
that changes per optimizer step is read ON THE DEVICE from a rate table indexed by the Adam step counter the kernels
already keep there (csrc/lr_table.h).  ``LrSchedule`` owns the user's torch scheduler and that table: before every
epoch it evaluates the actual scheduler - any ``torch.optim.lr_scheduler``, user-written ones included - into the
table, so the device needs no per-scheduler math and the rates are torch's, rounded once to fp32.

Table layout (one fp32 buffer, fixed address for the whole fit): words 0..3 ``{int32 t0, int32 len, 0, 0}``, words
4.. ``lr[0..len)``; ``lr[k]`` is the rate of the optimizer step that runs after ``t0 + k`` steps have been taken, the
index clamped to ``[0, len - 1]``.

Lightning's rules kept: interval ``"epoch"`` steps the scheduler after validation when ``(epoch + 1) % frequency ==
0``; interval ``"step"`` after the optimizer step of batch ``b`` when ``(b + 1) % frequency == 0`` (batch index inside
the epoch); ``ReduceLROnPlateau`` needs ``monitor`` and reads it from ``trainer.callback_metrics`` after validation.
"""
from __future__ import annotations

import warnings
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch
from torch.optim import lr_scheduler as _tls

TABLE_HEADER = 4  # words before lr[0] (csrc/lr_table.h LR_TABLE_HEADER)
INTERVALS = ("epoch", "step")
_SCHEDULER_KEYS = {"scheduler", "interval", "frequency", "monitor", "strict", "name"}
_BASE = getattr(_tls, "LRScheduler", None) or getattr(_tls, "_LRScheduler")


def _is_scheduler(obj) -> bool:
    return isinstance(obj, (_BASE, _tls.ReduceLROnPlateau))


def parse_configure_optimizers(result) -> Tuple[Any, Optional[Dict]]:
    """(optimizer, scheduler config or None) of a ``configure_optimizers()`` return value.

    Accepted, as in Lightning: an optimizer; ``[opt]`` / ``(opt,)``; ``([opt], [sched])``; ``{"optimizer": opt,
    "lr_scheduler": sched or dict}``.  The scheduler dict's keys: ``scheduler``, ``interval`` ("epoch"), ``frequency``
    (1), ``monitor``, ``strict`` (True), ``name``.  More than one optimizer or scheduler raises ValueError."""
    opt, sched = result, None
    if isinstance(result, dict):
        unknown = set(result) - {"optimizer", "lr_scheduler", "monitor"}
        if unknown or "optimizer" not in result:
            raise ValueError(f"configure_optimizers(): a dict needs 'optimizer' (and optionally 'lr_scheduler'); "
                             f"unexpected keys {sorted(unknown)}")
        opt, sched = result["optimizer"], result.get("lr_scheduler")
        if sched is not None and not isinstance(sched, dict) and result.get("monitor") is not None:
            sched = {"scheduler": sched, "monitor": result["monitor"]}
    elif (isinstance(result, (list, tuple)) and len(result) == 2
          and all(isinstance(x, (list, tuple)) for x in result)):
        opts, scheds = result
        if len(opts) != 1:
            raise ValueError(f"configure_optimizers() returned {len(opts)} optimizers: exactly one is supported")
        if len(scheds) > 1:
            raise ValueError(f"configure_optimizers() returned {len(scheds)} lr schedulers: at most one is supported")
        opt, sched = opts[0], (scheds[0] if scheds else None)
    elif isinstance(result, (list, tuple)):
        if len(result) != 1:
            raise ValueError(f"configure_optimizers() returned {len(result)} optimizers: exactly one is supported")
        opt = result[0]
        if isinstance(opt, dict):
            return parse_configure_optimizers(opt)
    if sched is None:
        return opt, None
    if isinstance(sched, (list, tuple)):
        if len(sched) != 1:
            raise ValueError(f"configure_optimizers() returned {len(sched)} lr schedulers: at most one is supported")
        sched = sched[0]
    cfg = dict(scheduler=sched) if not isinstance(sched, dict) else dict(sched)
    unknown = set(cfg) - _SCHEDULER_KEYS
    if unknown or "scheduler" not in cfg:
        raise ValueError(f"lr_scheduler dict needs 'scheduler' and takes {sorted(_SCHEDULER_KEYS)}; "
                         f"unexpected keys {sorted(unknown)}")
    cfg.setdefault("interval", "epoch")
    cfg.setdefault("frequency", 1)
    cfg.setdefault("monitor", None)
    cfg.setdefault("strict", True)
    cfg.setdefault("name", None)
    return opt, cfg


def plain_state(obj):
    """``obj`` with everything that is not a plain container, scalar, string or tensor replaced by None, so a scheduler
    state dict stays loadable under ``torch.load(weights_only=True)`` (torch's own state dicts already drop plain
    functions and keep a callable object's ``__dict__``; anything else in there that is not plain is dropped)."""
    if isinstance(obj, dict):
        return {k: plain_state(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(plain_state(v) for v in obj) if type(obj) in (list, tuple) else [plain_state(v) for v in obj]
    if obj is None or isinstance(obj, (bool, int, float, str, torch.Tensor)):
        return obj
    return None


class LrSchedule:
    """The scheduler of a fit and its per-step rates: a host list for the epoch, and on a GPU the device table.

    ``live=True`` (a torch optimizer stepped in Python, trainer/engines.py AutogradEngine without flat Adam): the real
    scheduler is stepped as the steps run, and the optimizer's own rate is what training uses; the host list only
    records the rates for logging."""

    def __init__(self, optimizer, scheduler, interval: str = "epoch", frequency: int = 1, monitor: Optional[str] = None,
                 strict: bool = True, name: Optional[str] = None, live: bool = False):
        if interval not in INTERVALS:
            raise ValueError(f"lr_scheduler interval must be one of {INTERVALS}, got {interval!r}")
        if int(frequency) < 1:
            raise ValueError(f"lr_scheduler frequency must be >= 1, got {frequency}")
        if not _is_scheduler(scheduler):
            raise ValueError(f"lr_scheduler: {type(scheduler).__name__} is not a learning-rate scheduler")
        if getattr(scheduler, "optimizer", optimizer) is not optimizer:
            raise ValueError("lr_scheduler: the scheduler is attached to another optimizer than the one returned")
        self.plateau = isinstance(scheduler, _tls.ReduceLROnPlateau)
        if self.plateau and monitor is None:
            raise ValueError("lr_scheduler: ReduceLROnPlateau needs 'monitor' (the metric it watches), e.g. "
                             "{'scheduler': sched, 'monitor': 'val_loss'}")
        if self.plateau and interval != "epoch":
            raise ValueError("lr_scheduler: ReduceLROnPlateau is stepped after validation (interval 'epoch'); "
                             "interval 'step' is not supported for it")
        if isinstance(scheduler, (_tls.OneCycleLR, _tls.CyclicLR)) and getattr(scheduler, "cycle_momentum", False):
            raise ValueError(f"lr_scheduler: {type(scheduler).__name__} with cycle_momentum=True also schedules "
                             "momentum / beta1, which is not supported: pass cycle_momentum=False")
        rates = {float(g["lr"]) for g in optimizer.param_groups}
        if len(rates) != 1:
            raise ValueError(f"lr_scheduler: parameter groups with different learning rates {sorted(rates)} are not "
                             "supported (one rate for the whole flat parameter buffer)")
        self.optimizer = optimizer
        self.scheduler = scheduler
        self.interval = interval
        self.frequency = int(frequency)
        self.monitor = monitor
        self.strict = bool(strict)
        self.name = name or f"lr-{type(optimizer).__name__}"
        self.live = bool(live)
        self.t0 = 0
        self.host: List[float] = [self.current_lr]  # rates of steps t0, t0 + 1, .. (clamped reads: rate_for)
        self.table: Optional[torch.Tensor] = None  # device table (GPU engines), fixed address once handed out
        self._bound = False

    @classmethod
    def from_config(cls, optimizer, cfg: Dict, live: bool = False) -> "LrSchedule":
        return cls(optimizer, cfg["scheduler"], cfg.get("interval", "epoch"), cfg.get("frequency", 1),
                   cfg.get("monitor"), cfg.get("strict", True), cfg.get("name"), live=live)

    # ------------------------------------------------------------------ rates
    @property
    def current_lr(self) -> float:
        return float(self.optimizer.param_groups[0]["lr"])

    def _advance(self, *args):
        """scheduler.step().  Training steps run on the device (or not yet, when a table is filled ahead), so torch's
        "`lr_scheduler.step()` before `optimizer.step()`" warning does not apply here: suppressed, calls not reordered."""
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message=r"Detected call of `lr_scheduler\.step\(\)` before")
            warnings.filterwarnings("ignore", message=r".*epoch parameter in `scheduler\.step\(\)`")
            self.scheduler.step(*args)

    def rate_for(self, taken: int) -> float:
        """Rate of the step that runs after ``taken`` steps: the device's clamped read of the table, on the host."""
        k = min(max(int(taken) - self.t0, 0), len(self.host) - 1)
        return self.host[k]

    def begin_epoch(self, taken: int, n_steps: int, device=None):
        """Before an epoch of ``n_steps`` optimizer steps, ``taken`` steps after the start of training: the rates of
        the epoch's steps on the host and (``device`` a GPU) in the device table.  Interval "step" advances the
        scheduler while filling - after the fill it stands where the epoch's last step leaves it; "epoch" writes the
        one rate of the epoch (every index clamps to it)."""
        self.t0 = int(taken)
        if self.live:
            self.host = []
        elif self.interval == "step":
            rates = []
            for b in range(int(n_steps)):
                rates.append(self.current_lr)
                if (b + 1) % self.frequency == 0:
                    self._advance()
            self.host = rates or [self.current_lr]
        else:
            self.host = [self.current_lr]
        if device is not None and torch.device(device).type == "cuda" and not self.live:
            self._upload(torch.device(device))

    def set_window(self, t0: int, rates: Sequence[float], device=None):
        """The table from rates given outright - ``rates[k]`` for the step after ``t0 + k`` steps - instead of from the
        scheduler (kernel tests and measurements)."""
        if not len(rates):
            raise ValueError("lr schedule: a window needs at least one rate")
        self.t0, self.host = int(t0), [float(r) for r in rates]
        if device is not None and torch.device(device).type == "cuda":
            self._upload(torch.device(device))

    def before_step(self):
        """live: the rate the optimizer step about to run uses (recorded for logging)."""
        if self.live:
            self.host.append(self.current_lr)

    def after_step(self, batch_idx: int):
        """live, interval "step": Lightning steps the scheduler after the optimizer step of batch ``batch_idx``."""
        if self.live and self.interval == "step" and (int(batch_idx) + 1) % self.frequency == 0:
            self._advance()

    def end_epoch(self, epoch: int, metrics: Optional[Dict[str, float]] = None):
        """After the epoch's validation: interval "epoch" steps the scheduler (ReduceLROnPlateau on its monitored
        metric; a missing metric raises with ``strict``, is skipped with a warning without)."""
        if self.interval != "epoch" or (int(epoch) + 1) % self.frequency != 0:
            return
        if self.plateau:
            value = (metrics or {}).get(self.monitor)
            if value is None:
                msg = (f"ReduceLROnPlateau conditioned on metric {self.monitor!r} which is not available; available "
                       f"metrics: {sorted(metrics or {})}")
                if self.strict:
                    raise RuntimeError(msg)
                warnings.warn(msg, RuntimeWarning)
                return
            self._advance(float(value))
        else:
            self._advance()

    # ------------------------------------------------------------------ device table
    def table_image(self) -> torch.Tensor:
        """The table as int32 words on the host: header {t0, len, 0, 0}, then the fp32 rates' bits."""
        n = len(self.host)
        img = torch.zeros(TABLE_HEADER + n, dtype=torch.int32)
        img[0], img[1] = self.t0, n
        img[TABLE_HEADER:] = torch.tensor(self.host, dtype=torch.float64).to(torch.float32).view(torch.int32)
        return img

    def _upload(self, device: torch.device):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("lr schedule: the device rate table is filled before a step is captured "
                               "(begin_epoch / set_window), not inside the capture")
        n = TABLE_HEADER + len(self.host)
        if self.table is None or self.table.device != device or self.table.numel() < n:
            if self._bound:
                raise RuntimeError(f"lr schedule: the device rate table ({self.table.numel() - TABLE_HEADER} entries) "
                                   f"is bound into launches and cannot grow to {n - TABLE_HEADER}")
            # buffers come 256-byte aligned from the caching allocator (the kernels read the header as one aligned word)
            self.table = torch.zeros(n, dtype=torch.float32, device=device)
        # A blocking copy from pageable memory, once per epoch: complete on return, so the replays / launches that
        # follow read the new window.  No pinned staging buffer is kept: the schedule hangs off the engine, which a
        # Trainer <-> module reference cycle hands to the garbage collector, and a pinned block released there records
        # an event on the stream of its last copy - an error if the collector happens to run inside a graph capture.
        # Only the current stream is synchronised: the engines drain their own streams at the end of an epoch (the
        # Trainer reads the epoch's losses back) before the next window is written over the last one.
        self.table.view(torch.int32)[:n].copy_(self.table_image())
        torch.cuda.current_stream(device).synchronize()

    def device_table(self, device) -> torch.Tensor:
        """The device table, for binding into a launch or a capture: from here on its address is fixed."""
        device = torch.device(device)
        if self.table is None or self.table.device != device:
            self._upload(device)
        self._bound = True
        return self.table

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict:
        """The scheduler's state for a checkpoint.  A step-interval scheduler is advanced for the whole epoch when the
        epoch's table is filled, so between begin_epoch and the epoch's end this state stands at the epoch's end;
        the Trainer writes checkpoints after an epoch, where the two agree."""
        return plain_state(self.scheduler.state_dict())

    def load_state(self, sd: Dict, param_group: Optional[Dict] = None):
        """Scheduler state of a checkpoint, and the optimizer param group's ``lr`` / ``initial_lr`` saved with it (the
        chainable schedulers compute the next rate from the group's current one)."""
        if param_group is not None:
            for g in self.optimizer.param_groups:
                for k in ("lr", "initial_lr"):
                    if k in param_group:
                        g[k] = float(param_group[k])
        self.scheduler.load_state_dict(sd)
        self.host = [self.current_lr]

    def param_group_overlay(self) -> Dict:
        """What a checkpoint's optimizer param group takes from the schedule: the current rate and ``initial_lr``."""
        g = self.optimizer.param_groups[0]
        out = {"lr": float(g["lr"])}
        if "initial_lr" in g:
            out["initial_lr"] = float(g["initial_lr"])
        return out

"""Python face of the fused MLP training kernels (csrc/mlp_fused.hip).

``FusedMLPKernel`` owns the launch plan of one MLP architecture and validates every operand
on the host before a launch (shape, dtype, device, contiguity, index ranges): the kernel
itself trusts its arguments.  Parameters, Adam moments and gradients are flat fp32 buffers
in torch ``state_dict`` order (``net.0.weight, net.0.bias, net.3.weight, ...``), which is
also the layout of the DDP gradient bucket and of the Lightning checkpoint.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from ._native import native, ptr, stream_handle

LOSS_KINDS = {"ce": 0, "mse": 1}
# exchange polling of the wave kernels (csrc/mlp_fused.h xg_poll): two pipelined sweeps in flight
# (profiles/xg_poll_pipelined_ab_r2.log; probe-then-sweep and sequential polls measured slower)
XG_POLL = 3


def mlp_num_params(dims: Sequence[int]) -> int:
    return sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))


TILE_BMAX = 1024  # largest per-rank batch of the batch-tiled trainer (csrc/mlp_tile.hip)


WAVE_TRAINERS = ("wave_single", "wave_rows")  # MlpPlan.trainer's names (csrc/mlp_select.h)
BLOCK5_TRAINERS = ("block5", "block5_b8")


def tile_supported(dims: Sequence[int]) -> bool:
    """The batch-tiled trainer's own shape check (csrc/mlp_tile.hip make_plan); no GPU needed."""
    return bool(native().mlp_tile_supported([int(d) for d in dims]))


def tile_window_ok(dims: Sequence[int], batch: int, accumulate: int) -> bool:
    """The batch-tiled trainer runs optimizer steps of ``accumulate`` micro-batches of ``batch`` rows for this
    architecture: its shape rule, and its own window predicate (csrc/mlp_select.h mlp_tile_window_ok: batch 1..1024,
    ``accumulate * ceil(batch / 32)`` slots within the cap).  No GPU needed."""
    return tile_supported(dims) and bool(native().mlp_tile_window_ok(int(batch), int(accumulate)))


def check_accumulate(accumulate, name: str = "accumulate") -> int:
    """Micro-batches per optimizer step as an int >= 1 (``Trainer(accumulate_grad_batches=)``, ``train(accumulate=)``);
    ValueError for a non-integer, a bool or a value < 1 - Lightning's dict schedule is not supported."""
    if isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1:
        raise ValueError(f"{name} must be an int >= 1, got {accumulate!r}")
    return accumulate


OPTIMIZERS = ("adam", "adamw", "sgd")  # train(optimizer=): torch.optim.Adam / AdamW / SGD (csrc/mlp_fused.h MlpOptimizer)


def check_optimizer(optimizer, weight_decay: float = 0.0, momentum: float = 0.0, dampening: float = 0.0,
                    nesterov: bool = False) -> str:
    """The optimizer name of a train launch, checked with torch's own rules for the two optimizers added to Adam:
    ValueError for an unknown name, a negative weight decay or momentum, and Nesterov momentum without a momentum or
    with dampening.  ``"adam"`` is passed through with nothing new refused."""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
    if optimizer == "adam":
        return optimizer
    if not float(weight_decay) >= 0.0:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")
    if optimizer == "sgd":
        if not float(momentum) >= 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if nesterov and (float(momentum) <= 0.0 or float(dampening) != 0.0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
    return optimizer


def _mix_hash(a, b, c):
    """csrc/mlp_fused_impl.h mix_hash on numpy uint32 arrays (wrapping arithmetic)."""
    import numpy as np

    u = np.uint32
    with np.errstate(over="ignore"):
        h = a * u(0x9E3779B1)
        h = h ^ ((b + u(0x7F4A7C15)) * u(0x85EBCA77))
        h = h ^ ((c + u(0x165667B1)) * u(0xC2B2AE3D))
        h = h ^ (h >> u(16))
        h = h * u(0x7FEB352D)
        h = h ^ (h >> u(15))
        h = h * u(0x846CA68B)
        h = h ^ (h >> u(16))
    return h


def dropout_keep_mask(seed: int, gstep: int, layer: int, n_rows: int, n_units: int, p: float) -> torch.Tensor:
    """Host mirror of the fused kernels' dropout mask: bool [n_rows, n_units], True = kept.

    Keyed by (seed, global step, hidden layer, row within the batch, unit) with the kernels' own
    integer arithmetic: ``mix_hash(seed + (b >> 6) * 0x9E3779B9, gstep, (layer * 64 + (b & 63)) * 65536 + o)``
    and ``u01(h) < p`` means dropped.  Rows < 64 are the key of every fused trainer; the batch-tiled
    trainer folds ``b >> 6`` into the hash's first argument for the rows above."""
    import numpy as np

    u = np.uint32
    b = np.arange(n_rows, dtype=np.uint32)[:, None]
    o = np.arange(n_units, dtype=np.uint32)[None, :]
    with np.errstate(over="ignore"):
        a = u(int(seed) & 0xFFFFFFFF) + (b >> u(6)) * u(0x9E3779B9)
        key = (u(int(layer)) * u(64) + (b & u(63))) * u(65536) + o
        h = _mix_hash(a, np.broadcast_to(u(int(gstep) & 0xFFFFFFFF), key.shape), key)
    u01 = (h >> u(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return torch.from_numpy(~(u01 < np.float32(p)))


def _wave_hash(key):
    """csrc/mlp_wave_impl.h wave_hash on numpy uint32 arrays (wrapping arithmetic)."""
    import numpy as np

    u = np.uint32
    with np.errstate(over="ignore"):
        key = key ^ (key >> u(16))
        key = key * u(0x7FEB352D)
        key = key ^ (key >> u(15))
        key = key * u(0x846CA68B)
        key = key ^ (key >> u(16))
    return key


def wave_dropout_keep_mask(seed: int, gstep: int, layer: int, n_rows: int, n_units: int, p: float) -> torch.Tensor:
    """Host mirror of the wave kernels' dropout mask (csrc/mlp_wave_impl.h: the single-wave kernel and
    the row-parallel kernels): bool [n_rows, n_units], True = kept.

    ``hkey = (seed * 0x9E3779B1) ^ (gstep * 0x85EBCA77)``, unit ``j`` of row ``b`` in hidden layer
    ``layer`` draws ``wave_hash(hkey ^ ((layer * 4096 + b * 64 + j) * 0xC2B2AE3D))`` and is dropped when
    the draw is below ``(uint32)(p * 2^32)`` with ``p`` the fp32 dropout rate, all in uint32 arithmetic."""
    import numpy as np

    u = np.uint32
    b = np.arange(n_rows, dtype=np.uint32)[:, None]
    j = np.arange(n_units, dtype=np.uint32)[None, :]
    with np.errstate(over="ignore"):
        hkey = (u(int(seed) & 0xFFFFFFFF) * u(0x9E3779B1)) ^ (u(int(gstep) & 0xFFFFFFFF) * u(0x85EBCA77))
        r = _wave_hash(hkey ^ ((u(int(layer)) * u(4096) + b * u(64) + j) * u(0xC2B2AE3D)))
    thr = int(float(np.float32(p)) * 4294967296.0)  # < 2^32 for every fp32 p < 1
    return torch.from_numpy(~(r.astype(np.uint64) < np.uint64(thr)))


def wave_supported(dims: Sequence[int], batch: int) -> bool:
    """The wave kernels' own shape / batch check (csrc/mlp_wave.hip); no GPU needed."""
    return bool(native().mlp_wave_supported([int(d) for d in dims], int(batch)))


def _table_ptr(lr_tab: Optional[torch.Tensor]) -> int:
    """Device pointer of a rate table (0: none), checked: cuda fp32, 4 header words and at least one rate."""
    if lr_tab is None:
        return 0
    if not (lr_tab.is_cuda and lr_tab.dtype == torch.float32 and lr_tab.is_contiguous() and lr_tab.numel() >= 5):
        raise ValueError("lr_tab must be a contiguous cuda fp32 rate table (4 header words + >= 1 rate)")
    return lr_tab.data_ptr()


def check_label_smoothing(label_smoothing) -> float:
    """``label_smoothing`` as a float in [0, 1) (torch's range without 1: a fully smoothed target has no label)."""
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing!r}")
    return eps


def check_class_weight(class_weight, num_classes: int) -> Optional[torch.Tensor]:
    """``class_weight`` (None, a sequence or a tensor) as a CPU fp32 [C] tensor: exactly ``num_classes`` finite,
    strictly positive weights - so that a batch with a live row always has a positive normaliser."""
    if class_weight is None:
        return None
    w = torch.as_tensor(class_weight).detach().to("cpu", torch.float32).reshape(-1)
    if w.numel() != int(num_classes):
        raise ValueError(f"class_weight needs exactly {int(num_classes)} weights, got {w.numel()}")
    if not bool(torch.isfinite(w).all()) or not bool((w > 0).all()):
        raise ValueError("class_weight must be finite and strictly positive")
    return w


def confusion_weight_sum(confusion: torch.Tensor, class_weight=None) -> float:
    """``W = sum_i w[y_i]`` of the rows an ``infer`` launch counted, from its int64 confusion matrix (rows = label):
    ``sum_c w[c] * (row sum c)`` in fp64 - exact for fp32 weights (``class_weight=None``: the row count)."""
    rows = confusion.sum(1).to(torch.float64)
    w = torch.ones_like(rows) if class_weight is None else torch.as_tensor(class_weight).detach().cpu().double()
    return float((w.reshape(-1) * rows).sum())


def weighted_infer_stats(loss_sum: float, correct: int, confusion: torch.Tensor, class_weight=None):
    """(weighted loss mean, correct, confusion) of an ``infer`` launch that ran with class weights / label smoothing.

    There statistic word 0 is the numerator ``sum_i num_i``; the normaliser needs no accumulator of its own, it is
    ``confusion_weight_sum``'s (``class_weight=None``: smoothing alone).  nan for a launch without a labelled row."""
    W = confusion_weight_sum(confusion, class_weight)
    return (loss_sum / W if W > 0 else float("nan")), correct, confusion


class FusedMLPKernel:
    def __init__(self, dims: Sequence[int], bmax: int):
        if bmax not in (4, 16, TILE_BMAX):
            raise ValueError("fused MLP kernel is instantiated for batch <= 4, <= 16 or <= 1024")
        self.dims = [int(d) for d in dims]
        if bmax == TILE_BMAX and not tile_supported(self.dims):
            raise ValueError("the batch-tiled trainer (batch 17..1024) does not take this architecture")
        self.bmax = bmax
        self._plan = None
        self._eval_plan = None
        self._tile_ws = None  # slot workspace of the batch-tiled trainer (csrc/mlp_tile.hip)
        self._infer_ws_buf = None  # slot workspace of the inference kernel's statistics (csrc/mlp_infer.hip)

    def _tile_args(self, device, batch: int = 0, accumulate: int = 1) -> dict:
        """The batch-tiled trainer's slot workspace (partial gradients per tile + the fold's arrival
        counter, zero between launches), allocated once for batches up to ``bmax``; a launch whose accumulation
        window needs more slots than that gets a larger one (launches bound earlier keep theirs alive)."""
        if not self.plan.use_tile:
            return {}
        n = int(native().mlp_tile_ws_floats(self.dims, max(self.bmax, 16)))
        if accumulate > 1:
            n = max(n, int(native().mlp_tile_ws_floats_accum(self.dims, int(batch), int(accumulate))))
        if self._tile_ws is None or self._tile_ws.device != device or self._tile_ws.numel() < n:
            self._tile_ws = torch.zeros(n, dtype=torch.float32, device=device)
        return dict(tile_ws=ptr(self._tile_ws), tile_ws_floats=self._tile_ws.numel())

    def _check_accumulate(self, accumulate, batch: int) -> dict:
        """The native argument of a launch over windows of ``accumulate`` micro-batches ({} for 1)."""
        if check_accumulate(accumulate) == 1:
            return {}
        if self.plan.trainer(int(batch), accumulate=accumulate) != "tile":
            raise ValueError("accumulate > 1 needs the batch-tiled trainer: a plan of bmax 1024 for an architecture it "
                             f"takes, and accumulate * ceil(batch / 32) <= {int(native().mlp_tile_max_slots())} slots")
        return dict(accumulate=accumulate)

    def _check_optimizer(self, optimizer, batch: int, weight_decay, momentum, dampening, nesterov, train: bool) -> dict:
        """The native arguments of a launch's optimizer ({} for Adam, and for a grad-mode launch, which applies none)."""
        if check_optimizer(optimizer, weight_decay, momentum, dampening, nesterov) == "adam" or not train:
            return {}
        if self.plan.trainer(int(batch), optimizer=optimizer) != "tile":
            raise ValueError(f"optimizer={optimizer!r} needs the batch-tiled trainer: a plan of bmax 1024 "
                             "(any batch 1..1024) for an architecture it takes")
        if optimizer == "sgd":
            return dict(optimizer="sgd", momentum=float(momentum), dampening=float(dampening), nesterov=bool(nesterov))
        return dict(optimizer="adamw")

    @staticmethod
    def _moments_of(opt_args: dict, m, v):
        """The moment buffers a launch that applies an optimizer binds: m and v for Adam / AdamW; for SGD the momentum
        buffer m alone, and not even that without momentum (what the launch does not read is passed as null)."""
        if opt_args.get("optimizer") == "sgd":
            m = m if opt_args["momentum"] != 0.0 else None
            if opt_args["momentum"] != 0.0 and m is None:
                raise ValueError("SGD with momentum needs the momentum buffer m")
            return m, None
        if opt_args and (m is None or v is None):  # (Adam: checked as it always was)
            raise ValueError("an AdamW launch needs the moment buffers m and v")
        return m, v

    @property
    def plan(self):
        if self._plan is None:
            self._plan = native().MlpPlan(self.dims, self.bmax)
        return self._plan

    def fused_update_supported(self, batch: int) -> bool:
        """True if the update-then-grad DDP step (one kernel per step) is available."""
        return self.plan.trainer(int(batch), mode=1, pending=True) == "wave_single"

    def dropout_mask(self, seed: int, gstep: int, layer: int, batch: int, p: float) -> torch.Tensor:
        """Host mirror of the mask a training launch of this plan draws for hidden layer ``layer`` at
        global step ``gstep``: bool [batch, dims[layer + 1]], True = kept.  The hash family is that of the
        trainer the plan names for this batch (``MlpPlan.trainer``): the wave kernels' for the two wave
        trainers, ``dropout_keep_mask`` for every other one."""
        if not 0 <= layer < len(self.dims) - 2:
            raise ValueError(f"hidden layer {layer} outside 0..{len(self.dims) - 3}")
        if not 1 <= batch <= self.bmax:
            raise ValueError(f"batch {batch} outside 1..{self.bmax}")
        mirror = wave_dropout_keep_mask if self.plan.trainer(int(batch)) in WAVE_TRAINERS else dropout_keep_mask
        return mirror(seed, gstep, layer, batch, self.dims[layer + 1], p)

    @property
    def eval_plan(self):
        """The evaluation kernel's layout: 16-row chunks, or 4-row chunks for the shapes whose 16-row
        layout overflows the LDS budget (``supported`` accepts those at batch <= 4 on their 4-row plan)."""
        if self._eval_plan is None:
            plan = native().MlpPlan(self.dims, 16)
            if not plan.eval_fits:
                small = native().MlpPlan(self.dims, 4)
                if small.eval_fits:
                    plan = small
            self._eval_plan = plan
        return self._eval_plan

    @staticmethod
    def supported(dims: Sequence[int], batch: int) -> bool:
        """Some fused trainer takes this architecture at this per-rank batch: the plan's own budget
        (csrc/mlp_fused.hip mlp_make_shape) up to batch 16, the batch-tiled trainer's above.  No GPU needed."""
        return bool(native().mlp_supported([int(d) for d in dims], int(batch)))

    # ------------------------------------------------------------------ checks
    def _check_params(self, *ts):
        P = mlp_num_params(self.dims)
        for t in ts:
            if t is None:
                continue
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == P):
                raise ValueError(f"flat parameter buffer must be contiguous cuda fp32 [{P}], got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")

    def _check_data(self, X, Y, idx, n_items):
        if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.stride(1) == 1):
            raise ValueError("X must be a cuda fp32 [N, D] row-major tensor")
        if X.shape[1] < self.dims[0]:
            raise ValueError(f"X has {X.shape[1]} features, model expects {self.dims[0]}")
        if not (Y.is_cuda and Y.dtype == torch.int32 and Y.is_contiguous() and Y.numel() == X.shape[0]):
            raise ValueError("Y must be cuda int32 [N]")
        if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() >= n_items):
            raise ValueError("idx must be cuda int32 with at least n_items entries")

    def _check_wloss(self, class_weight, label_smoothing, loss: str, device) -> dict:
        """The native arguments of a class-weighted / label-smoothed launch ({} when both are off)."""
        eps = check_label_smoothing(label_smoothing)
        if class_weight is None and eps == 0.0:
            return {}
        if loss != "ce":
            raise ValueError("class_weight / label_smoothing apply to the cross-entropy loss only")
        if class_weight is not None:
            C = self.dims[-1]
            if not (isinstance(class_weight, torch.Tensor) and class_weight.is_cuda and class_weight.device == device
                    and class_weight.dtype == torch.float32 and class_weight.is_contiguous()
                    and class_weight.numel() == C):
                raise ValueError(f"class_weight must be a contiguous cuda fp32 [{C}] tensor on the parameters' device")
        return dict(class_w=ptr(class_weight), label_smooth=eps)

    def _check_wloss_train(self, class_weight, label_smoothing, loss: str, device, batch: int) -> dict:
        args = self._check_wloss(class_weight, label_smoothing, loss, device)
        if args and self.plan.trainer(int(batch), weighted=True) != "tile":
            raise ValueError("class_weight / label_smoothing need the batch-tiled trainer: a plan of bmax 1024 "
                             "(any batch 1..1024) for an architecture it takes")
        return args

    # ------------------------------------------------------------------ launches
    def train(self, p, m, v, X, Y, idx, n_items: int, batch: int, steps: int, t0: int, lr: float,
              betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, dropout: float = 0.0,
              seed: int = 0, step_base: int = 0, loss_out: Optional[torch.Tensor] = None,
              loss: str = "ce", grad_out: Optional[torch.Tensor] = None, step_counter: Optional[torch.Tensor] = None,
              cursor: Optional[torch.Tensor] = None, prof: Optional[torch.Tensor] = None,
              pending: Optional[torch.Tensor] = None, stage: Optional[torch.Tensor] = None,
              stream: Optional[int] = None, xg=None, xg_timeout_s: float = 2.0,
              lr_tab: Optional[torch.Tensor] = None, class_weight: Optional[torch.Tensor] = None,
              label_smoothing: float = 0.0, accumulate: int = 1, optimizer: str = "adam", momentum: float = 0.0,
              dampening: float = 0.0, nesterov: bool = False):
        """Run ``steps`` fused optimizer steps (mode 0) or one gradient step (grad_out given).

        ``optimizer``: ``"adam"`` (torch.optim.Adam), or on the batch-tiled trainer's plan ``"adamw"``
        (torch.optim.AdamW: ``p *= 1 - lr_t * weight_decay``, then Adam on the undecayed gradient) and ``"sgd"``
        (torch.optim.SGD with ``momentum``, ``dampening``, ``nesterov`` and the coupled ``weight_decay``; ``betas`` /
        ``eps`` are ignored, ``m`` is the momentum buffer - overwritten with the gradient at step count 0, and not
        needed (None) without momentum - and ``v`` is not touched and may be None).  ``lr_t`` is ``lr_tab``'s rate when
        a table is bound.  A grad-mode launch applies no optimizer and ignores all of it.

        ``accumulate`` = K > 1 (Lightning's ``accumulate_grad_batches``; the batch-tiled trainer's plan only): an
        optimizer step is a window of K micro-batches of ``batch`` rows and applies ``(1 / K) * sum_kb grad(loss_kb)``,
        ``loss_kb`` the micro-batch's own mean - always 1 / K, also in a short last window.  ``n_items`` still counts
        rows; ``steps``, ``t0``, ``step_base``, the device counters, the cursor and ``loss_out`` count optimizer steps;
        the reported loss is the window's last live micro-batch's; micro-batch ``kb`` of step ``t`` draws the dropout
        mask of ``dropout_keep_mask(seed, t * K + kb, ...)``.

        ``class_weight`` (cuda fp32 [C], strictly positive) / ``label_smoothing`` (in [0, 1)): torch's
        ``F.cross_entropy(weight=, label_smoothing=)`` with its weighted-mean normaliser ``sum_i w[y_i]``; CE only,
        and only on the batch-tiled trainer's plan (``bmax=TILE_BMAX``, any batch 1..1024).

        ``lr_tab``: a device rate table (csrc/lr_table.h, trainer/lr_schedule.py) - every step takes its rate from the
        table's entry for the steps taken before it (t0 + s, or the device step counter's) instead of ``lr``.

        ``xg``: a native ``PeerExchange`` -> data-parallel steps with the gradient all-reduce done
        inside the kernel over peer-mapped receive buffers (see ``parallel.xgmi``)."""
        mode = 1 if grad_out is not None else 0
        need_mv = mode == 0 or pending is not None
        opt_args = self._check_optimizer(optimizer, batch, weight_decay, momentum, dampening, nesterov, mode == 0)
        if need_mv:
            m, v = self._moments_of(opt_args, m, v)
        self._check_params(p, m if need_mv else None, v if need_mv else None)
        if pending is not None and not (pending.is_cuda and pending.dtype == torch.int32):
            raise ValueError("pending must be a cuda int32 flag")
        self._check_data(X, Y, idx, n_items)
        if batch > self.bmax:
            raise ValueError(f"batch {batch} > kernel bmax {self.bmax}")
        wl_args = self._check_wloss_train(class_weight, label_smoothing, loss, p.device, batch)
        acc_args = self._check_accumulate(accumulate, batch)
        if steps < 1 or (cursor is None and (steps - 1) * batch * accumulate >= n_items):
            raise ValueError("steps do not match the index list")
        if cursor is not None and (mode != 1 or not (cursor.is_cuda and cursor.dtype == torch.int32)):
            raise ValueError("cursor (cuda int32) is only valid with grad_out")
        if mode == 1:
            P = mlp_num_params(self.dims)
            if not (grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.numel() >= P + 1):
                raise ValueError("grad_out must be cuda fp32 with P+1 entries (grads + loss)")
        if stage is not None and not (stage.is_cuda and stage.dtype == torch.int32 and stage.numel() >= 64 * 3):
            raise ValueError("stage must be a cuda int32 buffer of >= 192 entries")
        if step_counter is not None and not (step_counter.is_cuda and step_counter.dtype == torch.int32):
            raise ValueError("step_counter must be a cuda int32 scalar tensor")
        if loss_out is not None and not (loss_out.is_cuda and loss_out.dtype == torch.float32
                                         and loss_out.numel() >= steps):
            raise ValueError("loss_out must be cuda fp32 [steps]")
        xg_args = {}
        if xg is not None and xg.world > 1:
            if mode != 0 or cursor is not None or pending is not None or not self.xg_supported(batch, xg.world):
                raise ValueError("in-kernel all-reduce needs train mode on the single-wave 2-layer kernel or the "
                                 "3x128 block kernel (2 .. 8 ranks)")
            need = self.xg_buffer_bytes(xg.world, batch)
            if xg.bytes < need:
                raise ValueError(f"exchange buffer too small ({xg.bytes} < {need} bytes)")
            xg_args = dict(xg_recv=xg.recv, xg_peers=xg.peers, xg_world=xg.world, xg_rank=xg.rank,
                           xg_status=xg.status, xg_timeout=int(xg_timeout_s * 1e8), xg_poll=XG_POLL)
        self.plan.train(
            ptr(p), ptr(m) if need_mv else 0, ptr(v) if need_mv else 0, ptr(grad_out),
            ptr(X), X.stride(0), ptr(Y), ptr(idx), int(n_items), int(batch), int(steps), int(t0),
            float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(dropout),
            int(seed) & 0xFFFFFFFF, int(step_base) & 0xFFFFFFFF, ptr(loss_out), mode, LOSS_KINDS[loss],
            ptr(step_counter), ptr(cursor), ptr(prof), ptr(pending), ptr(stage),
            stream if stream is not None else stream_handle(),
            **xg_args, **self._tile_args(p.device, batch, accumulate), lr_tab=_table_ptr(lr_tab), **wl_args,
            **acc_args, **opt_args,
        )

    def prepare_train(self, p, m, v, X, Y, idx, n_items: int, batch: int, lr: float, betas=(0.9, 0.999),
                      eps: float = 1e-8, weight_decay: float = 0.0, dropout: float = 0.0, seed: int = 0,
                      loss_out: Optional[torch.Tensor] = None, loss: str = "ce",
                      step_counter: Optional[torch.Tensor] = None, xg=None, xg_timeout_s: float = 2.0,
                      xg_ticks: Optional[torch.Tensor] = None, lr_tab: Optional[torch.Tensor] = None,
                      class_weight: Optional[torch.Tensor] = None, label_smoothing: float = 0.0,
                      accumulate: int = 1, optimizer: str = "adam", momentum: float = 0.0, dampening: float = 0.0,
                      nesterov: bool = False) -> "BoundTrain":
        """Validate the operands of persistent train-mode launches ONCE and bind them natively.

        ``BoundTrain.run(first_step, steps)`` then launches steps [first_step, first_step+steps)
        over ``idx`` with losses in ``loss_out[first_step + s]`` - the per-launch cost is one
        positional native call (no keyword parsing, no tensor checks), which is what the short
        timed windows of the benchmark contract see.  ``accumulate`` as in ``train``: the steps are
        optimizer steps of ``accumulate`` micro-batches each.  ``optimizer`` / ``momentum`` / ``dampening`` /
        ``nesterov`` as in ``train``."""
        if not 1 <= batch <= self.bmax:
            raise ValueError(f"batch {batch} outside 1..{self.bmax}")
        opt_args = self._check_optimizer(optimizer, batch, weight_decay, momentum, dampening, nesterov, True)
        m, v = self._moments_of(opt_args, m, v)
        self._check_params(p, m, v)
        self._check_data(X, Y, idx, n_items)
        wl_args = self._check_wloss_train(class_weight, label_smoothing, loss, p.device, batch)
        acc_args = self._check_accumulate(accumulate, batch)
        if step_counter is None or not (step_counter.is_cuda and step_counter.dtype == torch.int32):
            raise ValueError("step_counter must be a cuda int32 scalar tensor (launches are step-relative)")
        if loss_out is not None and not (loss_out.is_cuda and loss_out.dtype == torch.float32
                                         and loss_out.is_contiguous()):
            raise ValueError("loss_out must be contiguous cuda fp32")
        xg_args = {}
        if xg is not None and xg.world > 1:
            if not self.xg_supported(batch, xg.world):
                raise ValueError("in-kernel all-reduce needs the single-wave 2-layer kernel or the 3x128 block "
                                 "kernel (2 .. 8 ranks)")
            need = self.xg_buffer_bytes(xg.world, batch)
            if xg.bytes < need:
                raise ValueError(f"exchange buffer too small ({xg.bytes} < {need} bytes)")
            xg_args = dict(xg_recv=xg.recv, xg_peers=xg.peers, xg_world=xg.world, xg_rank=xg.rank,
                           xg_status=xg.status, xg_timeout=int(xg_timeout_s * 1e8), xg_poll=XG_POLL)
            if xg_ticks is not None:
                if not (xg_ticks.is_cuda and xg_ticks.dtype == torch.int64 and xg_ticks.numel() >= 1):
                    raise ValueError("xg_ticks must be a cuda int64 counter")
                xg_args["xg_ticks"] = ptr(xg_ticks)
        launch = self.plan.prepare_train(
            ptr(p), ptr(m), ptr(v), ptr(X), X.stride(0), ptr(Y), ptr(idx), int(n_items), int(batch), float(lr),
            float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(dropout),
            int(seed) & 0xFFFFFFFF, ptr(loss_out), 0 if loss_out is None else loss_out.numel(), LOSS_KINDS[loss],
            ptr(step_counter), **xg_args, **self._tile_args(p.device, batch, accumulate), lr_tab=_table_ptr(lr_tab),
            **wl_args, **acc_args, **opt_args)
        return BoundTrain(launch, (p, m, v, X, Y, idx, loss_out, step_counter, xg, xg_ticks, self._tile_ws, lr_tab,
                                   class_weight),
                          p.device.index or 0)

    # ------------------------------------------------------------ in-kernel all-reduce
    def xg_slab_granules(self) -> int:
        """8-byte granules per (parity, source rank) slab of the exchange buffer (0 = unsupported)."""
        return int(native().mlp_xg_slab_granules(list(self.dims)))

    def xg_supported(self, batch: int, world: Optional[int] = None) -> bool:
        """True when training launches can average gradients INSIDE the kernel: the single-wave
        kernel's 2-layer nets (any 2..8 ranks), or the 3x128 block kernel (csrc/mlp_block5.hip:
        reduce-scatter + all-gather with sharded Adam or the one-hop exchange, 2 .. 8 ranks; ``world=None`` asks whether
        some world size qualifies).  Never with the batch-tiled trainer (batch > 16)."""
        return self._xg_trainer(batch, world if world is not None else 2) != "none"

    def _xg_trainer(self, batch: int, world: int) -> str:
        """The trainer of this plan's train-mode exchange launches at ``world`` ranks ("none": refused)."""
        if not 1 <= batch <= self.bmax or world < 2:
            return "none"
        return self.plan.trainer(int(batch), world=int(world))

    def _block5_bytes(self, batch: int, world: int) -> int:
        if self._xg_trainer(batch, world) not in BLOCK5_TRAINERS:
            return 0
        return int(native().mlp_block5_xg_bytes(list(self.dims), int(batch), int(world)))

    def xg_buffer_bytes(self, world: int, batch: int = 4) -> int:
        if self._xg_trainer(batch, world) in WAVE_TRAINERS:
            return 2 * world * self.xg_slab_granules() * 8
        return self._block5_bytes(batch, world)

    def evaluate(self, p, X, Y, idx, n_items: int, acc_out: torch.Tensor, loss: str = "ce",
                 logits_out: Optional[torch.Tensor] = None, grid: Optional[int] = None,
                 stream: Optional[int] = None):
        """acc_out[0] += sum of per-row loss, acc_out[1] += #correct (no reset)."""
        self._check_params(p)
        self._check_data(X, Y, idx, n_items)
        if not (acc_out.is_cuda and acc_out.dtype == torch.float32 and acc_out.numel() >= 2):
            raise ValueError("acc_out must be cuda fp32 [2]")
        if logits_out is not None and logits_out.numel() < n_items * self.dims[-1]:
            raise ValueError("logits_out too small")
        plan = self.eval_plan
        chunks = (n_items + plan.bmax - 1) // plan.bmax
        g = grid or max(1, min(chunks, 256))
        plan.eval(ptr(p), ptr(X), X.stride(0), ptr(Y), ptr(idx), int(n_items), LOSS_KINDS[loss],
                  ptr(acc_out), ptr(logits_out), int(g), stream if stream is not None else stream_handle())

    # ------------------------------------------------------------ batch-tiled inference
    @staticmethod
    def infer_supported(dims: Sequence[int]) -> bool:
        """The batch-tiled inference kernel (csrc/mlp_infer.hip) takes this architecture: 2 or 3 linear layers,
        D0 1..32, hidden widths multiples of 16 in 16..128, 2..4 classes.  No GPU needed."""
        return bool(native().mlp_infer_supported([int(d) for d in dims]))

    def _infer_ws(self, device, n: int) -> torch.Tensor:
        """The statistics' slot workspace (at most 4096 slots), allocated once and grown on demand."""
        need = int(native().mlp_infer_ws_bytes(self.dims, int(n))) // 8
        ws = self._infer_ws_buf
        if ws is None or ws.device != device or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.int64, device=device)
            self._infer_ws_buf = ws
        return ws

    def infer(self, p, X, n: int, idx: Optional[torch.Tensor] = None, Y: Optional[torch.Tensor] = None,
              loss: str = "ce", logits_out: Optional[torch.Tensor] = None, probs_out: Optional[torch.Tensor] = None,
              pred_out: Optional[torch.Tensor] = None, stats_out: Optional[torch.Tensor] = None, norm=None,
              grid: Optional[int] = None, stream: Optional[int] = None,
              class_weight: Optional[torch.Tensor] = None, label_smoothing: float = 0.0):
        """One forward-only launch over rows ``idx[0 .. n)`` of ``X`` (``idx=None``: rows ``0 .. n - 1``).

        Per-row outputs, each optional: ``logits_out`` / ``probs_out`` fp32 [n, C], ``pred_out`` int32 [n] (argmax,
        lowest index on ties).  ``norm=(mean, std)``: cuda fp32 [D0] each, the gather computes ``(x - mean) / std``
        (the caller replaces a zero std by 1).  With labels ``Y`` (int32, indexed like X's rows) the launch also
        writes ``stats_out``, ONE cuda int64 buffer of ``2 + C * C`` words: word 0 holds the bits of the fp64 loss sum
        (``stats_out[:1].view(torch.float64)``), word 1 the correct count, words ``2 + y * C + pred`` the confusion
        matrix (rows = label, columns = prediction); ``infer_stats`` unpacks it.  The statistics depend on the inputs
        and ``n`` only - not on ``grid``, not on the run.  Without ``Y`` nothing is written to ``stats_out``.

        ``class_weight`` (cuda fp32 [C]) / ``label_smoothing`` as in ``train`` (CE only): word 0 is then the numerator
        ``sum_i num_i`` of torch's weighted mean; ``weighted_infer_stats`` divides it by ``W``."""
        if not self.infer_supported(self.dims):
            raise ValueError(f"the inference kernel does not take the architecture {self.dims}")
        self._check_params(p)
        if p.data_ptr() % 16:
            raise ValueError("the flat parameter buffer must lie on a 16-byte boundary")
        n = int(n)
        C = self.dims[-1]
        if n < 1:
            raise ValueError("n must be >= 1")
        if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.stride(1) == 1):
            raise ValueError("X must be a cuda fp32 [N, D] row-major tensor")
        if X.shape[1] < self.dims[0]:
            raise ValueError(f"X has {X.shape[1]} features, model expects {self.dims[0]}")
        if idx is None:
            if n > X.shape[0]:
                raise ValueError(f"n = {n} rows asked of a table of {X.shape[0]}")
        elif not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() >= n):
            raise ValueError("idx must be cuda int32 with at least n entries")
        if Y is not None:
            if not (Y.is_cuda and Y.dtype == torch.int32 and Y.is_contiguous() and Y.numel() == X.shape[0]):
                raise ValueError("Y must be cuda int32 [N]")
            if stats_out is None or not (stats_out.is_cuda and stats_out.dtype == torch.int64
                                         and stats_out.is_contiguous() and stats_out.numel() >= 2 + C * C):
                raise ValueError(f"stats_out must be a contiguous cuda int64 buffer of >= {2 + C * C} words")
        for name, t, dt, cnt in (("logits_out", logits_out, torch.float32, n * C),
                                 ("probs_out", probs_out, torch.float32, n * C), ("pred_out", pred_out, torch.int32, n)):
            if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= cnt):
                raise ValueError(f"{name} must be a contiguous cuda {dt} buffer of >= {cnt} entries")
        mean = std = None
        if norm is not None:
            mean, std = norm
            for t in (mean, std):
                if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == self.dims[0]):
                    raise ValueError(f"norm = (mean, std) must be contiguous cuda fp32 [{self.dims[0]}] each")
        wl_args = self._check_wloss(class_weight, label_smoothing, loss, p.device)
        ws = self._infer_ws(p.device, n) if Y is not None else None
        native().mlp_infer(self.dims, ptr(p), ptr(X), X.stride(0), ptr(idx), ptr(Y), n, ptr(mean), ptr(std),
                           LOSS_KINDS[loss], ptr(logits_out), ptr(probs_out), ptr(pred_out), ptr(ws),
                           0 if ws is None else ws.numel() * 8, ptr(stats_out) if Y is not None else 0,
                           int(grid or 0), stream if stream is not None else stream_handle(), **wl_args)

    def infer_stats(self, stats_out: torch.Tensor):
        """(loss sum: float, correct: int, confusion: int64 [C, C] on the CPU) of an ``infer`` launch (one sync)."""
        C = self.dims[-1]
        host = stats_out[: 2 + C * C].cpu()
        return float(host[:1].view(torch.float64)[0]), int(host[1]), host[2:].reshape(C, C).clone()


# the current stream's raw handle without building a torch.cuda.Stream object (one C call); the
# public API is the fallback should the private binding go away
_raw_stream_fn = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_stream(device_index: int) -> int:
    if _raw_stream_fn is not None:
        return _raw_stream_fn(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


class BoundTrain:
    """A prepared persistent train launch (see ``FusedMLPKernel.prepare_train``).  Holds the
    bound tensors so their storage outlives every launch enqueued through it."""

    __slots__ = ("_launch", "_keep", "_dev", "n_items", "loss_len")

    def __init__(self, launch, keep, device_index: int):
        self._launch = launch
        self._keep = keep
        self._dev = device_index
        self.n_items = int(launch.n_items)
        self.loss_len = int(launch.loss_len)

    def run(self, first_step: int, steps: int, stream: Optional[int] = None):
        self._launch.run(first_step, steps, _raw_stream(self._dev) if stream is None else stream)


# ---------------------------------------------------------------------------- reference
def reference_mlp_forward(p: torch.Tensor, dims: Sequence[int], x: torch.Tensor) -> torch.Tensor:
    """Plain-torch fp32 forward of the flat-parameter MLP (no dropout), for numerics tests."""
    off = 0
    h = x
    L = len(dims) - 1
    for l in range(L):
        i, o = dims[l], dims[l + 1]
        W = p[off: off + i * o].view(o, i)
        off += i * o
        b = p[off: off + o]
        off += o
        h = h @ W.t() + b
        if l < L - 1:
            h = torch.relu(h)
    return h

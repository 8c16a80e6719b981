"""Step engines: how one training epoch / one optimizer step is executed.

* ``FusedMLPEngine`` (GPU, MLP family with widths that fit one CU): the reference's whole
  per-step hot loop (collate -> forward -> CE -> backward -> DDP all-reduce -> Adam,
  jobs/train_lightning_ddp.py:66-71,88,136) runs in the fused HIP kernels of
  csrc/mlp_fused.hip with the dataset resident in HBM and batches gathered on device.
    - world size 1: ONE persistent launch runs every step of an epoch (weights in LDS, Adam
      moments in VGPRs, nothing but the batch rows touches HBM per step).
    - world size > 1, 2-layer nets of the single-wave kernel (the reference model): the same
      persistent launch, with the DDP gradient average done INSIDE the kernel over xGMI peer
      mappings (parallel/xgmi.py) - one launch per rank per epoch, no per-step collective.
    - other world size > 1 cases: per step {fused fwd+bwd (grads + loss -> one flat buffer), RCCL
      ncclAvg all-reduce of that buffer (gradients AND the sync_dist train_loss in ONE
      collective: X5+X6 of SURVEY §2.6), fused flat Adam}; the epoch's step loop is captured
      once into a HIP graph and replayed every epoch (the Adam step count and dropout stream
      are read from a device counter, so replays are exact).
* ``AutogradEngine`` (any TrainModule; CPU/gloo plumbing path and the large-model GPU path):
  ``training_step`` + autograd, parameters/gradients as views of flat buffers, the bucketed
  reducer hooked on ``post_accumulate_grad`` (overlap with backward), flat Adam.

The fused engine applies torch.optim.Adam natively on every plan, and torch.optim.AdamW / SGD (optim_hparams_of) on the
batch-tiled trainer's plan (csrc/mlp_tile.hip: the optimizer is the fold kernel's), with flat SGD / flat Adam with
decoupled decay on its DDP step path; every other optimizer runs on the autograd engine as the torch optimizer itself.

A learning-rate scheduler returned by ``configure_optimizers()`` (trainer/lr_schedule.py) is followed by the autograd
all three engines (the graph engine: trainer/graph_engine.py): every launch that applies Adam reads the step's rate
from a device table at the device step count, so persistent launches and captured graphs follow a per-step schedule.
"""
from __future__ import annotations

import contextlib
import math
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..data.sampler import distributed_indices
from ..ops._native import reload_knobs
from ..ops.fused_mlp import (TILE_BMAX, FusedMLPKernel, check_accumulate, mlp_num_params, tile_supported,
                             tile_window_ok, weighted_infer_stats)
from ..ops.nn import BatchGather, bound_params, fold_batch_gather, join_side_work, unit_loss_seed
from ..ops.optim import FlatAdam, FlatSGD, _torch_adamw_group_defaults, adam_flat_, check_clip_args, sgd_flat_
from ..parallel.dist import DistContext, init_native_comm
from ..parallel.reducer import NativeBucketReducer, TorchBucketReducer, plan_buckets
from ..utils.debug import assert_reducer_complete, check_device
from ..utils.debug import enabled as debug_enabled
from ..utils.debug import reducer_timing_enabled
from .lr_schedule import LrSchedule, parse_configure_optimizers


def adam_hparams_from(optimizer) -> Optional[Dict]:
    """Extract Adam hyper-parameters from a configure_optimizers() result (None if not Adam).  ``lr`` is the rate the
    optimizer holds now; a returned lr scheduler is read by parse_configure_optimizers (trainer/lr_schedule.py)."""
    try:
        opt, _ = parse_configure_optimizers(optimizer)
    except ValueError:
        return None
    return adam_hparams_of(opt)


def adam_hparams_of(opt) -> Optional[Dict]:
    """Adam hyper-parameters of one optimizer (what parse_configure_optimizers returned), None if it is not Adam."""
    if type(opt) is not torch.optim.Adam:
        return None
    g = opt.param_groups[0]
    if g.get("amsgrad") or g.get("maximize"):
        return None
    return dict(lr=float(g["lr"]), betas=tuple(float(b) for b in g["betas"]), eps=float(g["eps"]),
                weight_decay=float(g["weight_decay"]))


def optim_hparams_of(opt) -> Optional[Dict]:
    """Hyper-parameters of an optimizer the fused engine applies natively, None for every other one (another class,
    ``amsgrad``, ``maximize``, param groups that differ): Adam's dict exactly as adam_hparams_of gives it (no ``kind``
    key), the same keys plus ``kind="adamw"`` for torch.optim.AdamW, and for torch.optim.SGD
    ``dict(kind="sgd", lr, momentum, dampening, nesterov, weight_decay)``."""
    if type(opt) is torch.optim.Adam:
        return adam_hparams_of(opt)
    if type(opt) not in (torch.optim.AdamW, torch.optim.SGD):
        return None
    g = opt.param_groups[0]
    keys = ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "momentum", "dampening", "nesterov")
    if g.get("amsgrad") or g.get("maximize") or any(h.get(k) != g.get(k) for h in opt.param_groups[1:] for k in keys):
        return None
    if type(opt) is torch.optim.AdamW:
        return dict(kind="adamw", lr=float(g["lr"]), betas=tuple(float(b) for b in g["betas"]), eps=float(g["eps"]),
                    weight_decay=float(g["weight_decay"]))
    return dict(kind="sgd", lr=float(g["lr"]), momentum=float(g["momentum"]), dampening=float(g["dampening"]),
                nesterov=bool(g["nesterov"]), weight_decay=float(g["weight_decay"]))


def spec_weighted(spec: Dict) -> bool:
    """A fused_spec() that asks for class weights or label smoothing (models/mlp.py carries the keys only when set)."""
    return spec.get("class_weight") is not None or float(spec.get("label_smoothing", 0.0)) != 0.0


class _EngineBase:
    name = "base"

    def __init__(self, model, ctx: DistContext, batch_size: int, seed: int):
        if ctx.device.type == "cuda":
            reload_knobs()  # bind time: the native launchers' DCT_* knobs
        self.model = model
        self.ctx = ctx
        self.B = int(batch_size)
        self.seed = int(seed)
        self.global_step = 0

    def epoch_local_indices(self, n_train: int, epoch: int, shuffle: bool) -> torch.Tensor:
        return distributed_indices(n_train, self.ctx.world_size, self.ctx.rank, shuffle=shuffle, seed=self.seed,
                                   epoch=epoch)


# ================================================================================ fused
class FusedMLPEngine(_EngineBase):
    name = "fused"
    epoch_engine = True  # runs whole epochs on device; the Trainer reads back per-step losses
    # DDP step path (the RCCL / peer-exchange fallback of the in-kernel exchange): steps per captured
    # graph chunk, and the update-then-grad single kernel where the wave kernel supports it (tests
    # override these on the class to exercise the other paths)
    GRAPH_CHUNK = 256
    FUSED_UPDATE = True

    @staticmethod
    def applicable(model, device: torch.device, batch_size: int, accumulate: int = 1, optimizer: str = "adam") -> bool:
        if device.type != "cuda" or not hasattr(model, "fused_spec"):
            return False
        spec = model.fused_spec()
        if optimizer != "adam" and accumulate <= 1:
            # AdamW / SGD: only the batch-tiled trainer's fold applies them, at any batch it takes
            if (spec_weighted(spec) and spec["loss"] != "ce") or not tile_supported(spec["dims"]):
                return False
            return 1 <= batch_size <= TILE_BMAX
        if accumulate > 1:
            # windows of micro-batches: only the batch-tiled trainer runs them - its shapes, any batch 1..1024,
            # accumulate * ceil(batch / 32) slots within its cap
            if (spec_weighted(spec) and spec["loss"] != "ce") or not tile_supported(spec["dims"]):
                return False
            return 1 <= batch_size <= TILE_BMAX and tile_window_ok(spec["dims"], batch_size, accumulate)
        if spec_weighted(spec):
            # class weights / label smoothing: only the batch-tiled trainer computes that loss, at any batch it takes
            return spec["loss"] == "ce" and tile_supported(spec["dims"]) and 1 <= batch_size <= TILE_BMAX
        return FusedMLPKernel.supported(spec["dims"], batch_size)

    def __init__(self, model, ctx: DistContext, batch_size: int, seed: int, adam: Dict,
                 steps_per_launch: int = 0, use_graph: Optional[bool] = None, lr_schedule=None,
                 accumulate_grad_batches: int = 1):
        super().__init__(model, ctx, batch_size, seed)
        # K = accumulate_grad_batches > 1: an optimizer step is a window of K micro-batches of B rows, one grid and one
        # fold of the batch-tiled trainer (csrc/mlp_tile.hip), so the kernel is built on the tile plan whatever the
        # batch.  Steps, losses, the device counters and the lr table count windows.  Under DDP the existing step path
        # runs once per window (grad-mode launch -> RCCL or the peer all-reduce + Adam -> flat Adam, HIP-graph chunks
        # included): one all-reduce per optimizer step, of the accumulated gradient; the tile plan has neither the
        # in-kernel exchange nor update-then-grad.
        self.K = check_accumulate(accumulate_grad_batches, "accumulate_grad_batches")
        self.acc = dict(accumulate=self.K) if self.K > 1 else {}
        # trainer/lr_schedule.py LrSchedule or None: every launch that applies Adam - the persistent trainers (with
        # and without the in-kernel exchange), the update-then-grad kernel, flat Adam and the peer all-reduce + Adam
        # of the DDP step path - reads the step's rate from its device table at the device step count
        self.lr_schedule = lr_schedule
        spec = model.fused_spec()
        self.dims = spec["dims"]
        self.dropout = float(spec["dropout"])
        self.loss = spec["loss"]
        self.adam = adam
        # the optimizer (optim_hparams_of: ``kind`` absent means Adam).  AdamW / SGD live in the batch-tiled trainer's
        # fold alone, so such a model is built on the tile plan whatever the batch, like a weighted loss or K > 1 -
        # without the in-kernel exchange, update-then-grad or the peer all-reduce + Adam kernel; its DDP step path is
        # grad-mode launch -> RCCL -> flat SGD / flat Adam with decoupled decay.  self.hp: the optimizer's keywords of a
        # train-mode launch
        self.kind = adam.get("kind", "adam")
        if self.kind == "sgd":
            self.hp = dict(lr=adam["lr"], weight_decay=adam["weight_decay"], optimizer="sgd",
                           momentum=adam["momentum"], dampening=adam["dampening"], nesterov=adam["nesterov"])
        else:
            self.hp = {k: adam[k] for k in ("lr", "betas", "eps", "weight_decay") if k in adam}
            if self.kind != "adam":
                self.hp["optimizer"] = self.kind
        # class-weighted / label-smoothed CE (models/mlp.py): the batch-tiled trainer's plan whatever the batch, and
        # the two arguments on every train launch; validation through the tiled inference kernel
        self.weighted = spec_weighted(spec)
        tiled = self.weighted or self.K > 1 or self.kind != "adam"
        bmax = TILE_BMAX if tiled else (4 if self.B <= 4 else (16 if self.B <= 16 else 1024))
        self.kernel = FusedMLPKernel(self.dims, bmax=bmax)
        if self.K > 1 and self.kernel.plan.trainer(self.B, accumulate=self.K) != "tile":
            raise ValueError(f"accumulate_grad_batches={self.K} at batch {self.B}: over the batch-tiled trainer's "
                             "slot cap (accumulate * ceil(batch / 32) <= 256)")
        self.P = mlp_num_params(self.dims)
        dev = ctx.device
        self.device = dev
        cw = spec.get("class_weight")
        self.class_weight = None if cw is None else torch.as_tensor(cw, dtype=torch.float32).contiguous().to(dev)
        self.wloss = {}
        if self.weighted:
            self.wloss = dict(class_weight=self.class_weight, label_smoothing=float(spec.get("label_smoothing", 0.0)))
        self.p = self._flat_from_model().to(dev)
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.step_counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps_per_launch = int(steps_per_launch)
        self.use_graph = (os.environ.get("DCT_GRAPH", "1") != "0") if use_graph is None else use_graph
        self.rank_seed = (self.seed * 1000003 + ctx.rank * 7919 + 1) & 0xFFFFFFFF
        self.comm = None
        self.gbuf = None
        # DDP step path; DCT_FORCE_DDP=1 drives it at world size 1 (single-GPU test of the
        # RCCL communicator + graph capture + device cursors)
        self.ddp = ctx.is_distributed or os.environ.get("DCT_FORCE_DDP", "0") == "1"
        self.fused_update = self.kernel.fused_update_supported(self.B) and self.FUSED_UPDATE  # (never on the tile plan)
        self.pending = torch.zeros(1, dtype=torch.int32, device=dev)
        self.stage = torch.zeros(64 * 4, dtype=torch.int32, device=dev)  # next-batch hand-off
        # (mlp_block5's grad mode takes no batch hand-off between DDP step launches: it measured 0.5 us
        # slower, profiles/block5_stage_ab_r3.log; the wave kernels' fused update uses self.stage)
        self._graphs = {}
        self.graph_chunk = int(self.GRAPH_CHUNK)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.graph_used = False
        if ctx.is_distributed:
            self.comm = init_native_comm(ctx) if ctx.backend == "nccl" else None
        elif self.ddp:
            from ..ops._native import native

            nat = native()
            self.comm = nat.Comm(nat.comm_unique_id(), 1, 0, dev.index or 0)
        if self.ddp:
            self.gbuf = torch.zeros(self.P + 1, dtype=torch.float32, device=dev)
            self._broadcast_params()
        self.xg = None  # in-kernel xGMI all-reduce (parallel/xgmi.py)
        self.gx = None  # DDP step path: fused peer all-reduce + Adam kernel over xGMI (csrc/xg_adam.hip)
        self._xg_probed = False
        if ctx.is_distributed:
            from ..parallel.xgmi import inkernel_enabled
            from ..parallel.xgmi import mode as xg_mode
            from ..parallel.xgmi import setup_grad_exchange, setup_peer_exchange, timeout_s

            # the persistent launch averages gradients itself when its kernel can (5-64-2 single-wave
            # kernel; the 3x128 block kernel at 2 .. 8 ranks) - the same answer on every rank, so
            # the collective setup below is entered by all or none
            if (self.kernel.xg_supported(self.B, ctx.world_size) and ctx.device.type == "cuda"
                    and inkernel_enabled()):
                self.xg = setup_peer_exchange(self.kernel, ctx, self.B)
            self.xg_timeout_s = timeout_s()
            # exchange time of the launches (s_memrealtime ticks, 100 MHz) -> allreduce_ms per epoch
            self.xg_ticks = torch.zeros(1, dtype=torch.int64, device=dev) if self.xg is not None else None
            if self.xg is None and not self.fused_update and self.kind == "adam":  # (xg_adam.hip applies Adam)
                self.gx = setup_grad_exchange(ctx, self.P + 1)
            if xg_mode() == "xgmi" and self.xg is None and self.gx is None:
                raise RuntimeError("DCT_ALLREDUCE=xgmi but neither the in-kernel exchange nor the peer "
                                   "all-reduce + Adam kernel is available for this model / world size")
            if self.xg is None and self.gx is None and self.comm is None:
                raise RuntimeError("distributed fused engine needs RCCL (backend nccl) or the in-kernel "
                                   "xGMI exchange; neither is available")
        elif self.ddp and not self.fused_update and self.kind == "adam" and os.environ.get("DCT_XG_GRAD") == "1":
            # single-GPU rehearsal (DCT_FORCE_DDP=1 DCT_XG_GRAD=1): the exchange kernel of one rank
            # (no pushes, no polls) in place of the one-rank RCCL all-reduce + flat Adam
            from ..ops._native import native
            from ..parallel.xgmi import timeout_s

            nat = native()
            self.gx = nat.PeerExchange(1, 0, nat.xg_adam_buffer_bytes(self.P + 1, 1))
            self.gx.set_peers([self.gx.recv])
            self.xg_timeout_s = timeout_s()
        self.last_allreduce_ms = None
        self._bound = None
        self._fast_run = None  # (loss_out, n_items, step limit, bound launch, loss ptr) of the last run

    # ------------------------------------------------------------------ params
    def _linear_params(self):
        out = []
        for lin in self.model.linear_layers():
            out += [lin.weight, lin.bias]
        return out

    def _flat_from_model(self) -> torch.Tensor:
        return torch.cat([t.detach().float().reshape(-1).cpu() for t in self._linear_params()])

    def _broadcast_params(self):
        if self.comm is None:  # gloo control plane (ranks sharing a device)
            self.ctx.broadcast_(self.p, src=0)
            return
        from ..ops._native import native

        nat = native()
        s = torch.cuda.current_stream().cuda_stream
        self.comm.broadcast(self.p.data_ptr(), self.P, nat.DT_F32, 0, s)  # X3 (DDP _sync_module_states)

    def sync_to_model(self):
        """Copy the flat device parameters back into the nn.Module (for checkpoints/serving)."""
        off = 0
        flat = self.p.detach().cpu()
        with torch.no_grad():
            for t in self._linear_params():
                n = t.numel()
                t.copy_(flat[off: off + n].view_as(t))
                off += n

    def load_from_model(self):
        self.p.copy_(self._flat_from_model().to(self.device))

    def _flat_optimizer(self):
        """The state-dict face of the optimizer in use, over this engine's buffers: torch's own layout - ``exp_avg`` /
        ``exp_avg_sq`` / ``step`` for Adam and AdamW (whose param-group keys are AdamW's), ``momentum_buffer`` for SGD."""
        shapes = [t.shape for t in self._linear_params()]
        a = self.adam
        if self.kind == "sgd":
            fo = FlatSGD(self.p, self.p, shapes, lr=a["lr"], momentum=a["momentum"], dampening=a["dampening"],
                         weight_decay=a["weight_decay"], nesterov=a["nesterov"], momentum_buffer=self.m)
            return fo
        fo = FlatAdam(self.p, self.p, shapes, lr=a["lr"], betas=a["betas"], eps=a["eps"],
                      weight_decay=a["weight_decay"])
        if self.kind == "adamw":
            group = _torch_adamw_group_defaults()
            group.update({k: fo.param_groups[0][k] for k in ("lr", "betas", "eps", "weight_decay", "params")})
            fo.param_groups = [group]
        fo.m, fo.v = self.m, self.v
        return fo

    def optimizer_state_dict(self) -> Dict:
        fo = self._flat_optimizer()
        fo.step_count = self.global_step
        return fo.state_dict()

    def load_optimizer_state(self, sd: Dict, global_step: int):
        fo = self._flat_optimizer()
        fo.load_state_dict(sd)
        self.global_step = global_step
        # (torch's SGD state carries no step count: the checkpoint's global_step is the count)
        self.step_counter.fill_(int(global_step if self.kind == "sgd" else fo.step_count))
        self._reset_exchanges()  # exchange tags derive from the step counter: drop stale granules

    def _reset_exchanges(self):
        """Collective: zero the exchanges' receive buffers (and status) once every rank is idle."""
        xs = [x for x in (self.xg, self.gx) if x is not None]
        if not xs:
            return
        torch.cuda.synchronize(self.device)
        self.ctx.barrier()
        for x in xs:
            x.reset(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize(self.device)
        self.ctx.barrier()

    # ------------------------------------------------------------------ data
    def attach_data(self, X: torch.Tensor, Y: torch.Tensor, train_rows: torch.Tensor, val_rows: torch.Tensor):
        dev = self.device
        if X.shape[1] != self.dims[0]:
            raise ValueError(f"dataset has {X.shape[1]} features, model expects {self.dims[0]}")
        self.X = X.to(torch.float32).contiguous().pin_memory().to(dev, non_blocking=True)
        self.Y = Y.to(torch.int32).contiguous().pin_memory().to(dev, non_blocking=True)
        n = X.shape[0]
        for rows in (train_rows, val_rows):
            if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
                raise ValueError("split indices out of range")
        self.train_rows = train_rows.to(torch.int64)
        self.val_rows = val_rows.to(torch.int64)
        n_local = math.ceil(len(self.train_rows) / self.ctx.world_size)
        self.idx = torch.zeros(max(1, n_local), dtype=torch.int32, device=dev)
        vl = math.ceil(max(1, len(self.val_rows)) / self.ctx.world_size)
        self.val_idx = torch.zeros(max(1, vl), dtype=torch.int32, device=dev)
        self.eval_acc = torch.zeros(2, dtype=torch.float32, device=dev)
        self._bound = None  # launches bound to the previous tables

    def steps_per_epoch(self) -> int:
        n_local = math.ceil(len(self.train_rows) / self.ctx.world_size)
        return math.ceil(n_local / (self.B * self.K))  # optimizer steps: windows of K batches

    def upload_epoch_indices(self, epoch: int, shuffle: bool = True) -> int:
        self.stage.zero_()  # staged batches refer to the previous index list
        local = self.epoch_local_indices(len(self.train_rows), epoch, shuffle)
        rows = self.train_rows[local].to(torch.int32)
        self.idx[: rows.numel()].copy_(rows.pin_memory(), non_blocking=True)
        return rows.numel()

    # ------------------------------------------------------------------ train
    def _lr_tab(self) -> Optional[torch.Tensor]:
        """The schedule's device table (bound from here on: a fixed address), or None."""
        return self.lr_schedule.device_table(self.device) if self.lr_schedule is not None else None

    def _bound_launch(self, n_items: int, loss_out: torch.Tensor):
        """The persistent train launch bound to (index list, loss buffer, exchange): validated once,
        then every run_steps call is one short native call (ops/fused_mlp.py BoundTrain)."""
        tab = self._lr_tab()
        key = (n_items, loss_out.data_ptr(), loss_out.numel(), 0 if tab is None else tab.data_ptr())
        bl = getattr(self, "_bound", None)
        if bl is None or self._bound_key != key:
            bl = self.kernel.prepare_train(self.p, self.m, self.v, self.X, self.Y, self.idx, n_items=n_items,
                                           batch=self.B, **self.hp, dropout=self.dropout, seed=self.rank_seed,
                                           loss_out=loss_out, loss=self.loss, step_counter=self.step_counter,
                                           xg=self.xg, xg_timeout_s=getattr(self, "xg_timeout_s", 20.0),
                                           xg_ticks=getattr(self, "xg_ticks", None) if self.xg is not None else None,
                                           lr_tab=tab, **self.wloss, **self.acc)
            self._bound, self._bound_key = bl, key
        return bl

    @property
    def step_mode(self) -> str:
        if self.xg is not None:
            return "fused-persistent+xgmi-inkernel-allreduce"
        if not self.ddp:
            return "fused-persistent"
        if self.gx is not None:
            return "fused-step+xgmi-allreduce-adam" + ("+graph" if self.use_graph else "")
        return "fused-step+rccl" + ("+graph" if self.use_graph else "")

    def run_steps(self, n_items: int, steps: int, loss_out: torch.Tensor, first_step: int = 0):
        """Enqueue ``steps`` optimizer steps over batches [first_step, first_step+steps) of self.idx.

        loss_out is indexed by the absolute batch index (loss_out[first_step + s]) and must hold
        first_step + steps entries (with DDP: the cross-rank mean loss).  No host synchronisation.
        With accumulate_grad_batches = K > 1 a step is a window of K batches: steps, first_step and loss_out count
        windows, and a window's loss is its last live micro-batch's."""
        fr = self._fast_run
        if (fr is not None and loss_out is fr[0] and n_items == fr[1] and 0 < steps and 0 <= first_step
                and first_step + steps <= fr[2] and fr[3] is self._bound and loss_out.data_ptr() == fr[4]):
            # repeat call on the same bound launch (the driver's timed window): checks already done
            fr[3].run(first_step, steps)
            return
        if steps <= 0:
            return
        rows = self.B * self.K  # index entries per optimizer step
        if (first_step + steps - 1) * rows >= n_items or loss_out.numel() < first_step + steps:
            raise ValueError("step range exceeds the epoch's batches / loss buffer")
        if not self.ddp or self.xg is not None:
            bl = self._bound_launch(n_items, loss_out)
            if not self.steps_per_launch:
                self._fast_run = (loss_out, n_items, min(loss_out.numel(), -(-n_items // rows)), bl,
                                  loss_out.data_ptr())
            chunk = self.steps_per_launch or steps
            s = 0
            while s < steps:
                k = min(chunk, steps - s)
                bl.run(first_step + s, k)
                s += k
            return
        self.cursor.fill_(first_step)
        C = min(self.graph_chunk, steps)
        full, rem = divmod(steps, C)
        done = 0
        if self.use_graph:
            g = self._get_graph(n_items, C, loss_out)
            if g is not None:
                for _ in range(full):
                    g.replay()
                done = full * C
                self.graph_used = True
        for _ in range(steps - done):
            self._ddp_step(n_items, loss_out)
        if self.fused_update:  # the last step's update is still pending: apply it
            self._flat_step()
            self.pending.zero_()
        # the last step's reduced loss is flushed by the next kernel; flush it here instead
        last = first_step + steps - 1
        loss_out[last: last + 1].copy_(self.gbuf[self.P: self.P + 1])

    def _ddp_step(self, n_items: int, loss_out: torch.Tensor):
        """One DDP step at the device cursor: fused fwd/bwd (grads + local loss -> gbuf) ->
        RCCL ncclAvg all-reduce of gbuf (X5 + X6 in one collective) -> fused flat Adam; with the
        peer exchange (self.gx) the last two are one kernel over the xGMI mappings."""
        from ..ops._native import native

        a = self.adam
        nat = native()
        stream = torch.cuda.current_stream().cuda_stream
        if self.fused_update:
            # one kernel: apply the previous step's (reduced) Adam update, then fwd/bwd
            self.kernel.train(self.p, self.m, self.v, self.X, self.Y, self.idx, n_items=n_items, batch=self.B,
                              steps=1, t0=0, lr=a["lr"], betas=a["betas"], eps=a["eps"],
                              weight_decay=a["weight_decay"], dropout=self.dropout, seed=self.rank_seed,
                              loss=self.loss, grad_out=self.gbuf, step_counter=self.step_counter,
                              cursor=self.cursor, loss_out=loss_out, pending=self.pending, stage=self.stage,
                              lr_tab=self._lr_tab(), **self.wloss)
            self.comm.allreduce(self.gbuf.data_ptr(), self.P + 1, nat.DT_F32, nat.OP_AVG, stream)
            return
        self.kernel.train(self.p, None, None, self.X, self.Y, self.idx, n_items=n_items, batch=self.B, steps=1,
                          t0=0, lr=a["lr"], dropout=self.dropout, seed=self.rank_seed, loss=self.loss,
                          grad_out=self.gbuf, step_counter=self.step_counter, cursor=self.cursor,
                          loss_out=loss_out, **self.wloss, **self.acc)
        if self.gx is not None:
            from ..parallel.xgmi import allreduce_adam_

            allreduce_adam_(self.gx, self.gbuf, self.p, self.m, self.v, self.P, self.step_counter, a["lr"],
                            a["betas"], a["eps"], a["weight_decay"], timeout=self.xg_timeout_s, lr_tab=self._lr_tab())
            return
        self.comm.allreduce(self.gbuf.data_ptr(), self.P + 1, nat.DT_F32, nat.OP_AVG, stream)
        self._flat_step()

    def _flat_step(self):
        """The DDP step path's optimizer on the all-reduced gradient in gbuf, at the device step count (which the
        grad-mode launch has advanced already): flat Adam, flat Adam with decoupled decay (AdamW) or flat SGD."""
        a = self.adam
        if self.kind == "sgd":
            sgd_flat_(self.p, self.gbuf[: self.P], self.m, 1, a["lr"], a["momentum"], a["dampening"], a["nesterov"],
                      a["weight_decay"], step_counter=self.step_counter, lr_tab=self._lr_tab())
            return
        adam_flat_(self.p, self.gbuf[: self.P], self.m, self.v, 1, a["lr"], a["betas"], a["eps"],
                   a["weight_decay"], decoupled=self.kind == "adamw", step_counter=self.step_counter,
                   lr_tab=self._lr_tab())

    def _get_graph(self, n_items: int, C: int, loss_out: torch.Tensor):
        key = (n_items, C, loss_out.data_ptr())
        if key in self._graphs:
            return self._graphs[key]
        from ..ops._native import native

        nat = native()
        # RCCL lazy init and kernel attribute setup must happen outside the capture
        if self.gx is None:
            scratch = torch.zeros(64, dtype=torch.float32, device=self.device)
            self.comm.allreduce(scratch.data_ptr(), 64, nat.DT_F32, nat.OP_SUM,
                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize(self.device)
        state = (self.p, self.m, self.v, self.step_counter, self.cursor, self.gbuf, loss_out, self.pending,
                 self.stage)
        saved = [t.clone() for t in state]
        # one eager step first (kernel attributes, RCCL channels), then roll the state back
        self._ddp_step(n_items, loss_out)
        torch.cuda.synchronize(self.device)
        for t, sv in zip(state, saved):
            t.copy_(sv)
        self._reset_exchanges()  # the rolled-back step counter re-issues the eager step's tags
        g = torch.cuda.CUDAGraph()
        try:
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                    for _ in range(C):
                        self._ddp_step(n_items, loss_out)
            torch.cuda.current_stream().wait_stream(s)
        except Exception as e:  # noqa: BLE001 - eager fallback keeps training correct
            print(f"[dct] HIP graph capture failed ({e!r}); DDP steps run eagerly", flush=True)
            g = None
        torch.cuda.synchronize(self.device)
        for t, sv in zip(state, saved):
            t.copy_(sv)
        self._graphs[key] = g
        return g

    def train_epoch(self, epoch: int, shuffle: bool = True) -> torch.Tensor:
        n_items = self.upload_epoch_indices(epoch, shuffle)
        steps = math.ceil(n_items / (self.B * self.K))
        loss_out = getattr(self, "_loss_buf", None)
        if loss_out is None or loss_out.numel() < steps:
            self._loss_buf = loss_out = torch.zeros(max(1, steps), dtype=torch.float32, device=self.device)
        first = 0
        if self.xg is not None or self.gx is not None:
            torch.cuda.synchronize(self.device)
            self.ctx.barrier()  # start the epoch's kernels together (the exchange spins are bounded)
            if not self._xg_probed:
                first = self._probe_exchange(n_items, steps, loss_out[:steps])
        if first < steps:
            self.run_steps(n_items, steps - first, loss_out[:steps], first_step=first)
        check_device("fused epoch")
        if self.gx is not None:
            self.xg_verify(fallback=False)
        elif self.xg is not None:
            self.xg_verify(fallback=False)
            # wave 0's exchange time over the epoch (the in-kernel all-reduce: X5 + X6 of SURVEY 2.6)
            self.last_allreduce_ms = float(self.xg_ticks.item()) / 1e5
            self.xg_ticks.zero_()
        self.global_step += steps
        return loss_out[:steps]

    def _probe_exchange(self, n_items: int, steps: int, loss_out: torch.Tensor) -> int:
        """First steps of a run through the peer exchange with a SHORT spin limit, then a
        collective check: if some rank cannot see its peers' writes (xGMI mapping, IPC mode), the
        job pays seconds, not the full timeout per launch, and continues on RCCL with every rank
        re-synced from rank 0.  Returns the steps of this epoch already applied."""
        from ..parallel.xgmi import probe_timeout_s

        self._xg_probed = True
        k = min(steps, 4)
        # a timed-out exchange may leave a step half applied (xg_adam: per block): every rank keeps
        # its pre-probe state to return to - replicas were identical before the probe
        snap = [t.clone() for t in (self.p, self.m, self.v, self.step_counter)]
        a = self.adam
        if self.xg is not None:
            self.kernel.train(self.p, self.m, self.v, self.X, self.Y, self.idx, n_items=n_items, batch=self.B,
                              steps=k, t0=0, lr=a["lr"], betas=a["betas"], eps=a["eps"],
                              weight_decay=a["weight_decay"], dropout=self.dropout, seed=self.rank_seed,
                              loss_out=loss_out, loss=self.loss, step_counter=self.step_counter, xg=self.xg,
                              xg_timeout_s=probe_timeout_s(), lr_tab=self._lr_tab(), **self.wloss)
        else:
            full, self.xg_timeout_s = self.xg_timeout_s, probe_timeout_s()
            try:
                self.run_steps(n_items, k, loss_out, first_step=0)
            finally:
                self.xg_timeout_s = full
        if self.xg_verify(fallback=True, snapshot=snap):
            return k
        return 0  # every rank is back at its pre-probe state: the epoch runs whole on RCCL

    def xg_verify(self, fallback: bool, snapshot=None) -> bool:
        """Collective check of the in-kernel exchange.  On a timeout either raise (training: the
        steps of that launch are incomplete) or, with ``fallback``, re-sync every rank from rank 0
        and continue on the RCCL step path (benchmarks)."""
        x = self.xg if self.xg is not None else self.gx
        if x is None:
            return True
        from ..parallel.xgmi import check

        st = check(x, self.ctx)
        if st == 0:
            return True
        msg = f"in-kernel xGMI all-reduce timed out (step tag {st & 0x7FFFFFFF})"
        if not fallback:
            raise RuntimeError(msg)
        if self.ctx.rank == 0:
            print(f"[dct] {msg}; re-syncing from rank 0 and falling back to RCCL", flush=True)
        self.xg_disable(snapshot)
        return False

    def device_barrier(self) -> bool:
        """Enqueue the in-kernel exchange's device-side barrier on the current stream (collective).
        False when the exchange is not active (the caller then uses the process-group barrier)."""
        x = self.xg if self.xg is not None else self.gx
        if x is None:
            return False
        from ..parallel.xgmi import device_barrier

        device_barrier(x, torch.cuda.current_stream(self.device).cuda_stream, self.xg_timeout_s)
        return True

    def xg_disable(self, snapshot=None):
        """Leave the in-kernel exchange: replicas re-synced from rank 0, RCCL step path from now on.
        ``snapshot`` (p, m, v, step_counter taken while the replicas were in sync) is restored on
        every rank first, so no half-applied step of a timed-out exchange survives."""
        self.xg = None
        self.gx = None
        self._bound = None
        self._graphs = {}  # captured with the exchange's kernels
        if self.comm is None:
            raise RuntimeError("in-kernel exchange disabled and no RCCL communicator is available to fall back to")
        torch.cuda.synchronize(self.device)
        if snapshot is not None:
            for t, sv in zip((self.p, self.m, self.v, self.step_counter), snapshot):
                t.copy_(sv)
        for t in (self.p, self.m, self.v, self.step_counter):
            self.ctx.broadcast_(t, src=0)
        torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ eval
    def validate(self, rows: Optional[torch.Tensor] = None, limit: Optional[int] = None) -> Tuple[float, float]:
        rows = self.val_rows if rows is None else rows
        local = distributed_indices(len(rows), self.ctx.world_size, self.ctx.rank, shuffle=False)
        if limit is not None:
            local = local[:limit]
        r = rows[local].to(torch.int32)
        if r.numel() == 0:
            return float("nan"), float("nan")
        if r.numel() > self.val_idx.numel():
            self.val_idx = torch.zeros(r.numel(), dtype=torch.int32, device=self.device)
        self.val_idx[: r.numel()].copy_(r)
        if self.weighted:
            # mlp_eval_kernel knows no weights: one launch of the tiled inference kernel over the shard, the weighted
            # mean sum_i num_i / sum_i w[y_i] of the whole shard, then the cross-rank mean as below
            stats = getattr(self, "_infer_stats", None)
            if stats is None:
                C = self.dims[-1]
                stats = self._infer_stats = torch.zeros(2 + C * C, dtype=torch.int64, device=self.device)
            self.kernel.infer(self.p, self.X, r.numel(), idx=self.val_idx, Y=self.Y, loss=self.loss, stats_out=stats,
                              **self.wloss)
            vl, correct, _ = weighted_infer_stats(*self.kernel.infer_stats(stats), self.class_weight)
            vals = self.ctx.all_reduce_mean(torch.tensor([vl, correct / r.numel()], dtype=torch.float64)).tolist()
            return vals[0], vals[1]
        self.eval_acc.zero_()
        self.kernel.evaluate(self.p, self.X, self.Y, self.val_idx, r.numel(), self.eval_acc, loss=self.loss)
        stats = self.eval_acc / float(r.numel())
        stats = self.ctx.all_reduce_mean(stats)
        vals = stats.cpu().tolist()
        return vals[0], vals[1]


# ============================================================================= autograd
class AutogradEngine(_EngineBase):
    name = "autograd"

    def __init__(self, model, ctx: DistContext, batch_size: int, seed: int, bucket_cap_bytes: int = 8 << 20,
                 first_bucket_bytes: int = 1 << 20, gradient_clip_val: Optional[float] = None,
                 gradient_clip_algorithm: str = "norm", optimizers=None, accumulate_grad_batches: int = 1):
        """``optimizers``: the model's configure_optimizers() result when the caller already has it (the Trainer, so
        that optimizer and lr scheduler are created once); None calls it here.

        ``accumulate_grad_batches`` = K > 1 (Lightning's automatic optimization): ``train_step`` is called once per
        micro-batch; gradients are zeroed at a window's first micro-batch only, every micro-batch's mean loss is
        backpropagated with the seed 1 / K, and the bucket reducer (one all-reduce per optimizer step: ``no_sync`` on
        the others), clipping, the optimizer and the scheduler hooks run only on the micro-batch that closes the window
        (``(batch_idx + 1) % K == 0``, or the epoch's last) - ``self.stepped`` tells the caller, and ``global_step``
        counts optimizer steps.  Such steps run eagerly: neither the captured step graph nor the device loop."""
        super().__init__(model, ctx, batch_size, seed)
        self.K = check_accumulate(accumulate_grad_batches, "accumulate_grad_batches")
        self.stepped = True  # the last train_step applied the optimizer (always, without accumulation)
        self._sync = True    # the gradient hooks hand buckets to the reducer (off while a window accumulates)
        # gradient clipping (Trainer(gradient_clip_val, gradient_clip_algorithm)): after the all-reduce, on the
        # averaged gradient, inside the flat Adam - p.grad keeps the unclipped gradient (ops/optim.py)
        self.clip_val, self.clip_algorithm = check_clip_args(gradient_clip_val, gradient_clip_algorithm)
        dev = ctx.device
        self.device = dev
        model.to(dev)
        params = [p for p in model.parameters() if p.requires_grad]
        self.params = params
        numels = [p.numel() for p in params]
        total = sum(numels)
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in params:
                n = p.numel()
                self.flat_p[off: off + n].copy_(p.detach().reshape(-1).float())
                p.data = self.flat_p[off: off + n].view_as(p)
                p.grad = self.flat_g[off: off + n].view_as(p)
                off += n
        if ctx.is_distributed:
            ctx.broadcast_(self.flat_p, 0) if ctx.backend != "nccl" else self._bcast_nccl()
        # models whose gradients become ready in block groups (the TabTransformer's grouped deferred
        # dW, model.ddp_block_groups) can get buckets aligned with the groups, each launched as its
        # group's dW launch is issued (DCT_TT_DDP_GROUPS=1).  Off by default: the step is graph-captured,
        # where the collectives run inline (runtime.cpp BucketReducer), so the split buys no overlap and
        # its second dW launch costs 7-14 us per step (forced-DDP TabTransformer 0.334-0.336 -> 0.322-0.327
        # ms, with the 60 us stand-in 0.397 -> 0.383-0.390; profiles/tt_ddp_groups_ab_r5.log)
        self._dw_groups, split_before = self._block_groups(model, params)
        self.plan = plan_buckets(numels, 4, bucket_cap_bytes, first_bucket_bytes, split_before=split_before)
        self.reducer = None
        # DCT_FORCE_DDP=1 at world size 1 on a GPU: the full DDP path (RCCL communicator of one
        # rank, bucket reducer on its comm stream, hooks, graph capture) - how its correctness,
        # overlap and cost are tested and measured on one GPU
        forced = (not ctx.is_distributed and dev.type == "cuda" and os.environ.get("DCT_FORCE_DDP", "0") == "1")
        if ctx.is_distributed or forced:
            if dev.type == "cuda" and (forced or ctx.backend == "nccl"):
                if forced:
                    from ..ops._native import native

                    nat = native()
                    self._own_comm = comm = nat.Comm(nat.comm_unique_id(), 1, 0, dev.index or 0)
                else:
                    comm = init_native_comm(ctx)
                # device-side all-reduce timing (allreduce_ms): opt-in (DCT_REDUCER_TIMING=1, or with
                # DCT_DEBUG=1) - its stamp kernels and the extra cross-stream edge cost every step,
                # so default training runs the same step the benchmark times; DCT_DEBUG=1 also adds
                # the stream-ordering check
                timing = reducer_timing_enabled()
                self.reducer = NativeBucketReducer(comm, self.flat_g, self.plan, timing=timing,
                                                   check=debug_enabled())
            else:
                # gloo: the CPU plumbing config, or GPU ranks sharing one device (init_distributed
                # falls back to gloo there because RCCL refuses it) - buckets staged through host
                # memory, which no HIP graph can capture
                staged = dev.type == "cuda"
                self.reducer = TorchBucketReducer(self.flat_g, self.plan, ctx.world_size, host_staging=staged)
                if staged:
                    self._graph_failed = True
            self._hooks = []
            for i, p in enumerate(params):
                self._hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(i)))
        self.graph_used = False
        # per-step GPU phase timing (device timestamps, works inside captured graphs): the Trainer
        # logs time/{fwd,bwd,allreduce,opt}_s per epoch
        self.phase_timer = None
        if dev.type == "cuda" and os.environ.get("DCT_PHASE_TIMING", "0") == "1":
            from ..utils.tracing import DevicePhaseTimer

            if self.K == 1:  # (an accumulating micro-batch has no all-reduce / optimizer phase to mark)
                self.phase_timer = DevicePhaseTimer(["fwd", "bwd", "allreduce", "opt"], dev)
        opt = model.configure_optimizers() if optimizers is None else optimizers
        torch_opt, sched_cfg = parse_configure_optimizers(opt)  # (parsed once: ValueError for what is not supported)
        hp = adam_hparams_of(torch_opt)
        # a returned lr scheduler (trainer/lr_schedule.py): with flat Adam its rates reach the kernel through the
        # device table (eager and captured steps) or as the step's scalar (CPU); with another torch optimizer the
        # real scheduler is stepped in Python beside it (live)
        self.lr_schedule = None
        if sched_cfg is not None:
            self.lr_schedule = LrSchedule.from_config(torch_opt, sched_cfg, live=hp is None)
        if hp is not None:
            self.optimizer = FlatAdam(self.flat_p, self.flat_g, [p.shape for p in params], clip_val=self.clip_val,
                                      clip_algorithm=self.clip_algorithm, lr_schedule=self.lr_schedule, **hp)
            self.torch_optimizer = None
        else:
            self.optimizer = None
            self.torch_optimizer = torch_opt
        # native-op fast paths (ops/nn.py bound_params): weight-gradient accumulation straight into
        # the flat bucket buffer, and bf16 shadow weights maintained by the fused Adam
        self._shadows = None
        self.flat_p16 = None
        if dev.type == "cuda" and self.optimizer is not None:
            self.flat_p16 = self.flat_p.to(torch.bfloat16)
            self.optimizer.p_bf16 = self.flat_p16
            self._shadows = {}
            off = 0
            for p in params:
                n = p.numel()
                self._shadows[id(p)] = self.flat_p16[off: off + n].view(p.shape)
                off += n

    def _bcast_nccl(self):
        self.ctx.broadcast_(self.flat_p, 0)

    def _block_groups(self, model, params):
        """(deferred-dW group sizes, bucket split indices) of a model with ddp_block_groups(), else
        ((), ()).  Only for data-parallel runs (a reducer to overlap with)."""
        groups = model.ddp_block_groups() if hasattr(model, "ddp_block_groups") else None
        dp = self.ctx.is_distributed or os.environ.get("DCT_FORCE_DDP", "0") == "1"
        if not groups or len(groups) < 2 or not dp or os.environ.get("DCT_TT_DDP_GROUPS", "0") != "1":
            return (), ()
        index = {id(p): i for i, p in enumerate(params)}
        splits = []
        for g in groups[:-1]:
            lo = min(g)  # the group's lowest block: its first parameter opens the bucket
            first = min(index[id(p)] for p in model.blocks[lo].parameters())
            splits.append(first - 1)
        return tuple(len(g) for g in groups), tuple(splits)

    def _make_hook(self, i):
        def hook(_p):
            if self._sync:
                self.reducer.mark_ready(i)
        return hook

    def attach_data(self, X: torch.Tensor, Y: torch.Tensor, train_rows: torch.Tensor, val_rows: torch.Tensor):
        self.X = X.to(self.device, torch.float32)
        self.Y = Y.to(self.device, torch.int64)
        self.train_rows = train_rows.to(torch.int64)
        self.val_rows = val_rows.to(torch.int64)

    def steps_per_epoch(self) -> int:
        return math.ceil(math.ceil(len(self.train_rows) / self.ctx.world_size) / (self.B * self.K))

    def _zero_grads(self):
        if self.flat_g.is_cuda:
            # a native kernel rather than zero_(): torch lowers it to a memset node, which replayed
            # graphs did not reliably order after the previous replay's Adam (csrc/step_kernels.hip)
            from ..ops._native import native

            native().zero_f32(self.flat_g.data_ptr(), self.flat_g.numel(), torch.cuda.current_stream().cuda_stream)
        else:
            self.flat_g.zero_()

    def _backward(self, loss: torch.Tensor):
        """loss.backward() with a persistent ones seed: autograd's implicit ones_like(loss) is a
        fill kernel per step (~4.5 us in the captured TabTransformer step on MI355X)."""
        one = getattr(self, "_one_seed", None)
        if one is None or one.device != loss.device or one.dtype != loss.dtype or one.shape != loss.shape:
            # (accumulate_grad_batches = K: every micro-batch's loss counts 1 / K)
            one = self._one_seed = torch.ones_like(loss) if self.K == 1 else torch.full_like(loss, 1.0 / self.K)
        loss.backward(one)
        join_side_work()  # weight-gradient GEMMs issued on the side stream (ops/nn.py side_dw)

    def _pm(self, i: int):
        """Phase mark i of the step (DCT_PHASE_TIMING=1): 0 start, 1 forward done, 2 backward done,
        3 all-reduce joined, 4 optimizer done."""
        if self.phase_timer is not None:
            self.phase_timer.mark(i)
            if i == 4:
                self.phase_timer.close()

    def _step_body(self, x, y, batch_idx: int, first: bool = True, step: bool = True):
        """One micro-batch.  ``first``: it opens its optimizer step (gradients are zeroed); ``step``: it closes it
        (reducer, clipping, optimizer, scheduler).  Both hold for every batch without accumulation."""
        if first:
            self._zero_grads()
        self._sync = step
        if self.reducer is not None and step:
            self.reducer.prepare()
        self._pm(0)
        self.model.train()
        # the step's backward root is training_step's loss with a seed of exactly 1 (_backward): a fused
        # classifier head may compute its backward inside the forward launch (ops/nn.py unit_loss_seed);
        # an accumulating step seeds 1 / K instead
        with self._bound(), (unit_loss_seed() if self.K == 1 else contextlib.nullcontext()):
            loss = self.model.training_step((x, y), batch_idx)
            if isinstance(loss, dict):
                loss = loss["loss"]
            self._pm(1)
            self._backward(loss)
        self._pm(2)
        if not step:
            return loss
        if self.K > 1:
            batch_idx = batch_idx // self.K  # the scheduler hook below counts optimizer steps
        if self.reducer is not None:
            self.reducer.finalize()
            assert_reducer_complete(self.reducer)
        self._pm(3)
        if self.optimizer is not None:
            self.optimizer.step()
        else:
            if self.clip_val is not None:
                if self.clip_algorithm == "norm":
                    norm = torch.nn.utils.clip_grad_norm_(self.params, self.clip_val)
                    self._torch_clip_stats = (norm, torch.clamp(self.clip_val / (norm + 1e-6), max=1.0))
                else:
                    torch.nn.utils.clip_grad_value_(self.params, self.clip_val)
            if self.lr_schedule is not None:
                self.lr_schedule.before_step()
            self.torch_optimizer.step()
            if self.lr_schedule is not None:
                self.lr_schedule.after_step(batch_idx)
        self._pm(4)
        return loss

    def grad_clip_stats(self) -> Tuple[float, float]:
        """(total gradient norm, clip coefficient) of the last step as Python floats; (nan, 1.0) when no norm is
        computed (clipping off or by value).  Synchronises: for tests and logging."""
        if self.optimizer is not None:
            return self.optimizer.clip_stats()
        st = getattr(self, "_torch_clip_stats", None)
        return (float(st[0]), float(st[1])) if st is not None else (float("nan"), 1.0)

    def train_step(self, rows: torch.Tensor, batch_idx: int, is_last: bool = False):
        """One optimizer step.  ``last_step_mode`` tells the Trainer how training_step ran:
        ``eager``; ``captured`` (traced into the step graph, then replayed - the tensors it logged
        are the graph's static outputs); ``replayed`` (training_step and self.log did NOT run).

        With accumulate_grad_batches = K > 1: one micro-batch, ``batch_idx`` its index in the rank's epoch and
        ``is_last`` set on the epoch's last one; the optimizer steps when ``(batch_idx + 1) % K == 0 or is_last``
        (``self.stepped``), always eagerly.  Returns the micro-batch's own (unscaled) loss."""
        rows_d = rows.to(self.device)
        self.last_step_mode = "eager"
        if self.K > 1:
            self.stepped = (batch_idx + 1) % self.K == 0 or bool(is_last)
            loss = self._step_body(self.X[rows_d], self.Y[rows_d], batch_idx, first=batch_idx % self.K == 0,
                                   step=self.stepped)
            self.global_step += int(self.stepped)
            return loss.detach()
        if self._graph_ok(rows_d.numel()):
            self.last_step_mode = "replayed" if getattr(self, "_graph", None) is not None else "captured"
            loss = self._graph_step(rows_d, batch_idx)
            if getattr(self, "_graph_failed", False):
                self.last_step_mode = "eager"
        elif getattr(self, "_warming", False):
            # graph warmup steps run on the capture stream (torch's capture recipe): autograd's
            # AccumulateGrad nodes then already live on that stream when the step is captured
            s = self._capture_stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                loss = self._step_body(self.X[rows_d], self.Y[rows_d], batch_idx).detach()
            torch.cuda.current_stream().wait_stream(s)
        else:
            loss = self._step_body(self.X[rows_d], self.Y[rows_d], batch_idx)
        self.global_step += 1
        return loss.detach()

    def _capture_stream(self):
        s = getattr(self, "_cap_stream", None)
        if s is None:
            self._cap_stream = s = torch.cuda.Stream(self.device)
        return s

    # ------------------------------------------------------------------ HIP graph of the step
    # GPU + flat Adam: after GRAPH_WARMUP eager steps the whole step (zero grads, forward,
    # backward with the bucket all-reduces issued from the grad hooks on the reducer's comm
    # stream, finalize, Adam with the device step counter) is captured once and replayed; the
    # batch is gathered into static input buffers by index_select on the device.
    GRAPH_WARMUP = 3

    def _graph_ok(self, n_rows: int) -> bool:
        self._warming = False
        if self.device.type != "cuda" or self.optimizer is None or n_rows != self.B:
            return False
        if os.environ.get("DCT_GRAPH", "1") == "0" or getattr(self, "_graph_failed", False):
            return False
        self._eager_full = getattr(self, "_eager_full", 0)
        if getattr(self, "_graph", None) is None and self._eager_full < self.GRAPH_WARMUP:
            self._eager_full += 1
            self._warming = True
            return False
        return True

    def _graph_step(self, rows_d: torch.Tensor, batch_idx: int):
        if getattr(self, "_graph", None) is None:
            self._x_static = self.X[rows_d].clone()
            self._y_static = self.Y[rows_d].clone()
            g = torch.cuda.CUDAGraph()
            try:
                s = self._capture_stream()
                s.wait_stream(torch.cuda.current_stream())
                torch.cuda.synchronize(self.device)
                with torch.cuda.stream(s):
                    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                        self._loss_static = self._step_body(self._x_static, self._y_static, batch_idx).detach()
                torch.cuda.current_stream().wait_stream(s)
            except Exception as e:  # noqa: BLE001 - eager steps stay correct
                print(f"[dct] HIP graph capture of the autograd step failed ({e!r}); running eagerly", flush=True)
                self._graph_failed = True
                torch.cuda.synchronize(self.device)
                return self._step_body(self.X[rows_d], self.Y[rows_d], batch_idx)
            self._graph = g
            self.graph_used = True
            # capture records without executing: Adam's host count moved, the device one did not
            self.optimizer.step_count -= 1
        torch.index_select(self.X, 0, rows_d, out=self._x_static)
        torch.index_select(self.Y, 0, rows_d, out=self._y_static)
        self._graph.replay()
        self.optimizer.step_count += 1
        return self._loss_static

    # ------------------------------------------------------------------ device-side batch loop
    # Steps over a device-resident list of dataset rows with NO host work between replays: the
    # captured graph starts with ONE prologue kernel (batch gather at the device cursor, Adam
    # step counter += 1, gradient zeroing) and ends with the Adam kernel, which also records the
    # step's loss at loss_out[cursor] and advances the cursor (csrc/step_kernels.hip,
    # csrc/optim.hip).  Replaces, per step: host batch slicing, two index_selects, a counter add,
    # a zero kernel and the loss copy.
    def device_loop_ok(self) -> bool:
        return (self.K == 1 and self.device.type == "cuda" and self.optimizer is not None and self.X.dim() == 2
                and self.X.shape[1] % 4 == 0 and os.environ.get("DCT_GRAPH", "1") != "0"
                and not getattr(self, "_graph_failed", False))

    def run_device_steps(self, rows_dev: torch.Tensor, first_step: int, steps: int, loss_out: torch.Tensor):
        """Steps first_step .. first_step + steps - 1 over rows_dev (int64, device) batches of B;
        losses land in loss_out[step] (fp32, device)."""
        if not self.device_loop_ok():
            for s in range(first_step, first_step + steps):
                loss_out[s] = self.train_step(rows_dev[s * self.B:(s + 1) * self.B], s)
            return
        from ..ops._native import native

        nat = native()
        s = first_step
        end = first_step + steps
        while s < end and getattr(self, "_dgraph", None) is None and self._eager_full_dev() < self.GRAPH_WARMUP:
            loss_out[s] = self.train_step(rows_dev[s * self.B:(s + 1) * self.B], s)  # warm-up (capture stream)
            s += 1
        if s >= end:
            return
        key = (rows_dev.data_ptr(), rows_dev.numel(), loss_out.data_ptr(), loss_out.numel())
        if getattr(self, "_dgraph", None) is None or self._dgraph_key != key:
            try:
                self._capture_device_graph(nat, rows_dev, loss_out, s)
            except Exception as e:  # noqa: BLE001 - eager steps stay correct
                print(f"[dct] HIP graph capture of the device-loop step failed ({e!r}); running eagerly", flush=True)
                self._graph_failed = True
                self._dgraph = None
                torch.cuda.synchronize(self.device)
                for t in range(s, end):
                    loss_out[t] = self.train_step(rows_dev[t * self.B:(t + 1) * self.B], t)
                return
            self._dgraph_key = key
        self._dcursor.fill_(s)
        # one replay per step: a graph holding 8 steps measured the same 0.420 ms/step on the
        # TabTransformer (profiles/tt_device_loop_chunk_ab_r2.log), the replays are already queued
        # back to back
        for _ in range(end - s):
            self._dgraph.replay()
        self.optimizer.step_count += end - s
        self.global_step += end - s

    def _eager_full_dev(self) -> int:
        return getattr(self, "_eager_full", 0)

    def _prologue(self, nat, rows_dev):
        st = torch.cuda.current_stream().cuda_stream
        nat.ag_step_prologue(self.X.data_ptr(), self.X.shape[1] * 4, self.Y.data_ptr(), rows_dev.data_ptr(),
                             self._dcursor.data_ptr(), self.B, rows_dev.numel(), self._x_dev.data_ptr(),
                             self._y_dev.data_ptr(), self.optimizer._device_counter().data_ptr(),
                             self.flat_g.data_ptr(), self.flat_g.numel(), st)

    def _capture_device_graph(self, nat, rows_dev, loss_out, first):
        if not (self.X.is_contiguous() and self.Y.is_contiguous() and self.X.dtype == torch.float32):
            raise RuntimeError("device loop needs contiguous fp32 features / int64 labels")
        self._x_dev = torch.empty(self.B, self.X.shape[1], dtype=torch.float32, device=self.device)
        self._y_dev = torch.empty(self.B, dtype=torch.int64, device=self.device)
        self._dcursor = torch.full((1,), first, dtype=torch.int32, device=self.device)
        # a model whose first fused block can gather its own batch (models/tabtransformer.py
        # folds_batch_gather) takes the step prologue into that launch; if no block took it, the step is
        # captured again with the prologue kernel
        fold = bool(getattr(self.model, "folds_batch_gather", False))
        for folded in ((True, False) if fold else (False,)):
            spec = None
            if folded:
                spec = BatchGather(self.X, rows_dev, self._dcursor, self.B, rows_dev.numel(), self._x_dev, self.Y,
                                   self._y_dev, self.optimizer._device_counter(), self.flat_g)
            g, loss = self._capture_step(nat, rows_dev, loss_out, first, spec)
            self.optimizer.step_count -= 1  # capture recorded without executing
            if spec is None or spec.consumed:
                break
        self.gather_folded = spec is not None and spec.consumed
        self._dgraph = g
        self._dloss = loss
        self.graph_used = True

    def _capture_step(self, nat, rows_dev, loss_out, first, spec):
        g = torch.cuda.CUDAGraph()
        s = self._capture_stream()
        s.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize(self.device)
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                if spec is None:
                    self._prologue(nat, rows_dev)
                if self.reducer is not None:
                    self.reducer.prepare()
                self._pm(0)
                self.model.train()
                with self._bound(), unit_loss_seed():  # (as _step_body: the backward seed is exactly 1)
                    with fold_batch_gather(spec) if spec is not None else contextlib.nullcontext():
                        loss = self.model.training_step((self._x_dev, self._y_dev), first)
                    if isinstance(loss, dict):
                        loss = loss["loss"]
                    self._pm(1)
                    self._backward(loss)
                self._pm(2)
                if self.reducer is not None:
                    self.reducer.finalize()
                self._pm(3)
                self.optimizer.step(bump_counter=False, epilogue=(self._dcursor, loss.detach(), loss_out))
                self._pm(4)
        torch.cuda.current_stream().wait_stream(s)
        return g, loss

    def optimizer_state_dict(self) -> Dict:
        if self.optimizer is not None:
            return self.optimizer.state_dict()
        return self.torch_optimizer.state_dict()

    def load_optimizer_state(self, sd: Dict, global_step: int):
        if self.optimizer is not None:
            self.optimizer.load_state_dict(sd)
        else:
            self.torch_optimizer.load_state_dict(sd)
        self.global_step = global_step

    def _bound(self):
        if self._shadows is None:
            return contextlib.nullcontext()
        # every transformer block's dW GEMMs as ONE grouped launch after backward (DCT_TT_DW_DEFER=0
        # keeps one launch per block): TabTransformer step 0.421-0.426 -> 0.407 ms
        # (profiles/tt_dw_defer_ab_r2.log).  With the native bucket reducer too: its hooks then only
        # count and every bucket launches at finalize, after the grouped launch - the model's
        # gradients fit ONE bucket (<= first_bucket_bytes), which could only start after the last
        # dW GEMM anyway, so deferring loses no overlap and keeps the grouped-dW win at W > 1
        defer_ok = self.reducer is None or isinstance(self.reducer, NativeBucketReducer)
        defer = defer_ok and os.environ.get("DCT_TT_DW_DEFER", "1") != "0"
        groups = self._dw_groups if (defer and self.reducer is not None) else ()
        if isinstance(self.reducer, NativeBucketReducer):
            # with block groups every group's dW launch is issued before its bucket's last hook
            # fires, so the hooks launch the buckets; otherwise they launch at finalize
            self.reducer.defer_launch = defer and self._has_deferrable_ops() and not groups
        return bound_params(self.params, self._shadows, defer_dw=defer, defer_groups=groups)

    def _has_deferrable_ops(self) -> bool:
        """True when the model routes weight gradients through the deferred grouped dW path
        (the fused transformer blocks); plain MLP/linear models keep hook-driven bucket launches."""
        return bool(getattr(self.model, "uses_fused_blocks", False))

    def sync_to_model(self):
        pass  # parameters ARE views of the flat buffer

    def load_from_model(self):
        # parameters ARE views of the flat buffer; only the bf16 shadow must follow external writes
        if self.flat_p16 is not None:
            self.flat_p16.copy_(self.flat_p)

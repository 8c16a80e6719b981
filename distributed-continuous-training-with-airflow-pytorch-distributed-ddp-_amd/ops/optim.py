"""Flat-buffer Adam (reference: ``torch.optim.Adam(self.parameters(), lr=0.01)``,
jobs/train_lightning_ddp.py:87-88).

Every parameter of the model is a view into ONE flat fp32 buffer (and every ``.grad`` a view
into one flat gradient buffer, which is what the bucketed reducer all-reduces), so a step
is one fused kernel launch on the GPU (csrc/optim.hip) or one vectorised torch expression on
the CPU plumbing path.  ``state_dict()`` emits exactly torch.optim.Adam's format so the
Lightning checkpoint's ``optimizer_states`` entry stays loadable by torch 2.1 / Lightning 2.1.

``sgd_flat_`` / ``FlatSGD`` are the same for ``torch.optim.SGD`` (momentum, dampening, Nesterov, coupled weight decay):
the flat step of the fused engine's DDP step path for an SGD model, and torch's ``momentum_buffer`` state layout.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from ._native import native, ptr, stream_handle


CLIP_ALGORITHMS = ("norm", "value")


def check_clip_args(clip_val, clip_algorithm: str):
    """(clip_val or None, algorithm) of ``gradient_clip_val`` / ``gradient_clip_algorithm`` as Lightning reads them:
    None or 0 is off; a negative value or an unknown algorithm raises ValueError."""
    if clip_algorithm not in CLIP_ALGORITHMS:
        raise ValueError(f"gradient_clip_algorithm must be one of {CLIP_ALGORITHMS}, got {clip_algorithm!r}")
    if clip_val is None:
        return None, clip_algorithm
    clip_val = float(clip_val)
    if not clip_val >= 0.0:
        raise ValueError(f"gradient_clip_val must be >= 0, got {clip_val}")
    return (clip_val or None), clip_algorithm


def clip_workspace(device) -> torch.Tensor:
    """Zeroed fp32 words of the norm kernel (csrc/optim.hip): {norm, coef, ticket, pad, one partial per workgroup}.
    Allocated once per optimizer: a captured step graph needs static addresses, and the ticket stays 0 between
    launches."""
    n = 4 + (native().grad_clip_workspace_floats() if torch.device(device).type == "cuda" else 0)
    return torch.zeros(n, dtype=torch.float32, device=device)


def grad_clip_coef_(g: torch.Tensor, max_norm: float, ws: torch.Tensor, grad_scale: float = 1.0) -> torch.Tensor:
    """ws[0:2] = {norm, coef} of ``torch.nn.utils.clip_grad_norm_(.., max_norm)`` over the flat gradient ``g`` scaled by
    ``grad_scale``: norm = sqrt(sum (grad_scale g)^2), coef = min(max_norm / (norm + 1e-6), 1).  ``g`` is not
    rewritten - the Adam step multiplies the coefficient in.  On the GPU one kernel, nothing read back; returns
    ws[0:2] (``ws``: clip_workspace())."""
    if g.dtype != torch.float32 or not g.is_contiguous() or ws.device != g.device or ws.dtype != torch.float32:
        raise ValueError("grad_clip_coef_: g and ws must be contiguous fp32 on one device")
    if not max_norm >= 0.0:
        raise ValueError("grad_clip_coef_: max_norm must be >= 0")
    if g.is_cuda:
        native().grad_clip_coef(ptr(g), g.numel(), float(grad_scale), float(max_norm), ptr(ws[4:]), ptr(ws[2:]),
                                ptr(ws), stream_handle(g.device))
    else:
        norm = g.norm() * abs(float(grad_scale))
        ws[0] = norm
        ws[1] = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return ws[:2]


def adam_flat_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr: float,
               betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, grad_scale: float = 1.0,
               decoupled: bool = False, p_bf16: Optional[torch.Tensor] = None,
               step_counter: Optional[torch.Tensor] = None, clip_coef: Optional[torch.Tensor] = None,
               clip_value: float = 0.0, lr_tab: Optional[torch.Tensor] = None):
    """In-place Adam on flat fp32 buffers; ``step`` is the 1-based step count after this update.  ``clip_coef`` (a
    one-element fp32 tensor on p's device, grad_clip_coef_'s ws[1:2]) is multiplied into ``grad_scale``;
    ``clip_value`` > 0 clamps the scaled gradient to [-clip_value, clip_value].  ``g`` is not rewritten.
    ``lr_tab`` (GPU, with ``step_counter``): a device rate table (csrc/lr_table.h, trainer/lr_schedule.py) - the step's
    rate is its entry for ``*step_counter - 1`` steps taken instead of ``lr``."""
    n = p.numel()
    for t in (g, m, v):
        if t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous() or t.device != p.device:
            raise ValueError("adam_flat_: p/g/m/v must be contiguous fp32 buffers of equal size on one device")
    if p.is_cuda:
        if p_bf16 is not None and (p_bf16.dtype != torch.bfloat16 or p_bf16.numel() != n):
            raise ValueError("p_bf16 must be a bf16 buffer of the same size")
        if step_counter is not None and not (step_counter.is_cuda and step_counter.dtype == torch.int32):
            raise ValueError("step_counter must be a cuda int32 tensor")
        if lr_tab is not None and (step_counter is None or not lr_tab.is_cuda or lr_tab.dtype != torch.float32
                                   or lr_tab.numel() < 5):
            raise ValueError("lr_tab must be a cuda fp32 rate table (4 header words + >= 1 rate) used with step_counter")
        if clip_coef is not None or clip_value:
            native().adam_flat_step_clipped(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), n, float(lr),
                                            float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                            max(1, int(step)), float(grad_scale), int(decoupled), ptr(step_counter),
                                            0, 0, 0, 0, ptr(clip_coef), float(clip_value), stream_handle(p.device),
                                            ptr(lr_tab))
            return
        native().adam_flat(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), n, float(lr), float(betas[0]),
                           float(betas[1]), float(eps), float(weight_decay), max(1, int(step)), float(grad_scale),
                           int(decoupled), ptr(step_counter), stream_handle(p.device), ptr(lr_tab))
        return
    if lr_tab is not None:
        raise ValueError("adam_flat_: a rate table is read on the GPU; on the CPU pass the step's rate as lr")
    b1, b2 = betas
    gg = g * grad_scale if grad_scale != 1.0 else g
    if clip_coef is not None:
        gg = gg * clip_coef  # (torch multiplies even by 1.0: exact)
    if clip_value:
        gg = gg.clamp(-clip_value, clip_value)
    if decoupled:
        p.mul_(1 - lr * weight_decay)
    elif weight_decay:
        gg = gg + weight_decay * p
    m.mul_(b1).add_(gg, alpha=1 - b1)
    v.mul_(b2).addcmul_(gg, gg, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = (v.sqrt() / (bc2 ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)
    if p_bf16 is not None:
        p_bf16.copy_(p)


def _torch_adam_group_defaults() -> Dict:
    """The param-group keys the installed ``torch.optim.Adam`` writes (they vary by torch
    version, e.g. ``decoupled_weight_decay`` since 2.6), so our optimizer state dicts stay
    loadable by ``torch.optim.Adam.load_state_dict`` and by Lightning."""
    try:
        d = dict(torch.optim.Adam([torch.zeros(1, requires_grad=True)]).defaults)
    except Exception:  # noqa: BLE001
        d = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None)
    return d


class FlatAdam:
    """Adam over a flat parameter buffer, torch.optim.Adam-compatible state_dict."""

    def __init__(self, flat_param: torch.Tensor, flat_grad: torch.Tensor, param_shapes: Sequence[torch.Size],
                 lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, clip_val: Optional[float] = None, clip_algorithm: str = "norm",
                 lr_schedule=None):
        if amsgrad:
            raise NotImplementedError("amsgrad is not supported")
        self.clip_val, self.clip_algorithm = check_clip_args(clip_val, clip_algorithm)
        # {norm, coef, ..} of the last step (clipping by norm): allocated here, once - static addresses for a capture
        self.clip_ws: Optional[torch.Tensor] = None
        if self.clip_val is not None and self.clip_algorithm == "norm":
            self.clip_ws = clip_workspace(flat_param.device)
        self.p = flat_param
        self.g = flat_grad
        self.m = torch.zeros_like(flat_param)
        self.v = torch.zeros_like(flat_param)
        self.shapes = [torch.Size(s) for s in param_shapes]
        group = _torch_adam_group_defaults()
        group.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                     params=list(range(len(self.shapes))))
        self.param_groups = [group]
        self.step_count = 0
        self.p_bf16: Optional[torch.Tensor] = None
        # trainer/lr_schedule.py LrSchedule (or None: the constant param-group rate).  On the GPU the kernels read the
        # step's rate from its device table at the device step count (a captured step follows the schedule); on the
        # CPU the step gets that same rate as the scalar.
        self.lr_schedule = lr_schedule

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    def step(self, grad_scale: float = 1.0, bump_counter: bool = True, epilogue=None):
        """One update.  ``bump_counter=False``: a step-prologue kernel already advanced the device
        step counter.  ``epilogue=(cursor, loss, loss_out)``: the Adam kernel also records
        loss_out[*cursor] = loss and advances the device batch cursor (graph-replayed loops)."""
        self.step_count += 1
        g = self.param_groups[0]
        counter = None
        if self.p.is_cuda:
            # the Adam step count lives on the device (advanced by a kernel, read by the Adam
            # kernel), so a captured step graph replays with the right bias correction
            counter = self._device_counter()
            if bump_counter:
                counter.add_(1)
        lr, lr_tab = g["lr"], None
        if self.lr_schedule is not None:
            if self.p.is_cuda:
                lr_tab = self.lr_schedule.device_table(self.p.device)
            else:
                lr = self.lr_schedule.rate_for(self.step_count - 1)
        clip_coef, clip_value = None, 0.0
        if self.clip_val is not None:
            # the gradient is clipped inside Adam (flat_g keeps the unclipped values): by norm, one kernel leaves the
            # coefficient on the device for the Adam launch behind it - no host round trip, graph-replayable
            if self.clip_algorithm == "norm":
                clip_coef = grad_clip_coef_(self.g, self.clip_val, self.clip_ws, grad_scale)[1:]
            else:
                clip_value = self.clip_val
        if epilogue is not None and self.clip_val is not None:
            cursor, loss, loss_out = epilogue
            b1, b2 = g["betas"]
            native().adam_flat_step_clipped(ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), ptr(self.p_bf16),
                                            self.p.numel(), float(lr), float(b1), float(b2), float(g["eps"]),
                                            float(g["weight_decay"]), max(1, self.step_count), float(grad_scale), 0,
                                            ptr(counter), ptr(cursor), ptr(loss), ptr(loss_out), loss_out.numel(),
                                            ptr(clip_coef), float(clip_value), stream_handle(self.p.device),
                                            ptr(lr_tab))
            return
        if epilogue is not None:
            cursor, loss, loss_out = epilogue
            b1, b2 = g["betas"]
            native().adam_flat_step(ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), ptr(self.p_bf16),
                                    self.p.numel(), float(lr), float(b1), float(b2), float(g["eps"]),
                                    float(g["weight_decay"]), max(1, self.step_count), float(grad_scale), 0,
                                    ptr(counter), ptr(cursor), ptr(loss), ptr(loss_out), loss_out.numel(),
                                    stream_handle(self.p.device), ptr(lr_tab))
            return
        adam_flat_(self.p, self.g, self.m, self.v, self.step_count, lr, g["betas"], g["eps"],
                   g["weight_decay"], grad_scale=grad_scale, p_bf16=self.p_bf16, step_counter=counter,
                   clip_coef=clip_coef, clip_value=clip_value, lr_tab=lr_tab)

    def clip_stats(self):
        """(norm, coef) of the last step's clipping by norm as Python floats (synchronises: tests and logging);
        (nan, 1.0) when nothing computes a norm (clipping off or by value)."""
        if self.clip_ws is None:
            return float("nan"), 1.0
        norm, coef = self.clip_ws[:2].tolist()
        return norm, coef

    def _device_counter(self) -> torch.Tensor:
        c = getattr(self, "_counter", None)
        if c is None or c.device != self.p.device:
            self._counter = c = torch.full((1,), self.step_count - 1, dtype=torch.int32, device=self.p.device)
        return c

    def sync_device_counter(self):
        """Re-seed the device step counter from the host count (after a state load)."""
        if self.p.is_cuda:
            self._device_counter().fill_(self.step_count)

    def zero_grad(self):
        self.g.zero_()

    # ------------------------------------------------------------------ state dict
    def _views(self, flat):
        out, off = [], 0
        for s in self.shapes:
            n = s.numel()
            out.append(flat[off: off + n].view(s))
            off += n
        return out

    def state_dict(self) -> Dict:
        state = {}
        if self.step_count > 0:
            ms, vs = self._views(self.m), self._views(self.v)
            for i in range(len(self.shapes)):
                state[i] = {
                    "step": torch.tensor(float(self.step_count)),
                    "exp_avg": ms[i].detach().to("cpu", torch.float32).clone(),
                    "exp_avg_sq": vs[i].detach().to("cpu", torch.float32).clone(),
                }
        groups = []
        for g in self.param_groups:
            gg = dict(g)
            gg["betas"] = tuple(gg["betas"])
            groups.append(gg)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd: Dict):
        pg = sd["param_groups"][0]
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k in pg:
                self.param_groups[0][k] = tuple(pg[k]) if k == "betas" else pg[k]
        st = sd.get("state", {})
        if st:
            ms, vs = self._views(self.m), self._views(self.v)
            steps = set()
            for i in range(len(self.shapes)):
                s = st[i] if i in st else st[str(i)]
                ms[i].copy_(s["exp_avg"])
                vs[i].copy_(s["exp_avg_sq"])
                steps.add(int(float(s["step"])))
            self.step_count = max(steps)
        else:
            self.step_count = 0
        if getattr(self, "_counter", None) is not None:
            self._counter.fill_(self.step_count)


# ---------------------------------------------------------------------------------------------- SGD
def sgd_flat_(p: torch.Tensor, g: torch.Tensor, m: Optional[torch.Tensor], step: int, lr: float,
              momentum: float = 0.0, dampening: float = 0.0, nesterov: bool = False, weight_decay: float = 0.0,
              grad_scale: float = 1.0, step_counter: Optional[torch.Tensor] = None,
              lr_tab: Optional[torch.Tensor] = None, epilogue=None):
    """In-place ``torch.optim.SGD`` (maximize=False) on flat fp32 buffers; ``m`` is the momentum buffer (None allowed
    without momentum) and ``step`` the 1-based step count after this update: at step 1 torch has no buffer yet, so the
    buffer becomes the gradient and what ``m`` held is ignored.  On the GPU one kernel (csrc/optim.hip); with
    ``step_counter`` (a cuda int32 that already includes this step) the count, and ``lr_tab``'s rate for
    ``*step_counter - 1`` steps taken, are read on the device.  ``epilogue=(cursor, loss, loss_out)`` as FlatAdam.step.
    ``g`` is not rewritten."""
    n = p.numel()
    momentum, dampening, weight_decay = float(momentum), float(dampening), float(weight_decay)
    if not momentum >= 0.0:
        raise ValueError(f"Invalid momentum value: {momentum}")
    if not weight_decay >= 0.0:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")
    if nesterov and (momentum <= 0.0 or dampening != 0.0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")
    if momentum != 0.0 and m is None:
        raise ValueError("sgd_flat_: momentum needs the buffer m")
    for t in (g, m):
        if t is not None and (t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous()
                              or t.device != p.device):
            raise ValueError("sgd_flat_: p/g/m must be contiguous fp32 buffers of equal size on one device")
    if p.is_cuda:
        if step_counter is not None and not (step_counter.is_cuda and step_counter.dtype == torch.int32):
            raise ValueError("step_counter must be a cuda int32 tensor")
        if lr_tab is not None and (step_counter is None or not lr_tab.is_cuda or lr_tab.dtype != torch.float32
                                   or lr_tab.numel() < 5):
            raise ValueError("lr_tab must be a cuda fp32 rate table (4 header words + >= 1 rate) used with step_counter")
        cursor, loss, loss_out = epilogue if epilogue is not None else (None, None, None)
        native().sgd_flat_step(ptr(p), ptr(g), ptr(m) if momentum != 0.0 else 0, n, float(lr), momentum, dampening,
                               bool(nesterov), weight_decay, max(1, int(step)), float(grad_scale), ptr(step_counter),
                               ptr(cursor), ptr(loss), ptr(loss_out), 0 if loss_out is None else loss_out.numel(),
                               stream_handle(p.device), ptr(lr_tab))
        return
    if lr_tab is not None or epilogue is not None:
        raise ValueError("sgd_flat_: a rate table / step epilogue is the GPU kernel's; on the CPU pass the rate as lr")
    gg = g * grad_scale if grad_scale != 1.0 else g
    if weight_decay:
        gg = gg + weight_decay * p
    if momentum != 0.0:
        if int(step) <= 1:
            m.copy_(gg)
        else:
            m.mul_(momentum).add_(gg, alpha=1 - dampening)
        gg = gg.add(m, alpha=momentum) if nesterov else m
    p.add_(gg, alpha=-lr)


def _torch_sgd_group_defaults() -> Dict:
    """The param-group keys the installed ``torch.optim.SGD`` writes (as _torch_adam_group_defaults)."""
    try:
        d = dict(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=1e-3).defaults)
    except Exception:  # noqa: BLE001
        d = dict(lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, maximize=False, foreach=None,
                 differentiable=False, fused=None)
    return d


def _torch_adamw_group_defaults() -> Dict:
    """The param-group keys the installed ``torch.optim.AdamW`` writes (as _torch_adam_group_defaults)."""
    try:
        d = dict(torch.optim.AdamW([torch.zeros(1, requires_grad=True)]).defaults)
    except Exception:  # noqa: BLE001
        d = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None)
    return d


class FlatSGD:
    """SGD over a flat parameter buffer, torch.optim.SGD-compatible state_dict: a per-parameter ``momentum_buffer``,
    present only with momentum and once a step has been taken.  torch's SGD state has no step count: the holder's
    ``step_count`` is the caller's to carry (the engines keep it as ``global_step``)."""

    def __init__(self, flat_param: torch.Tensor, flat_grad: torch.Tensor, param_shapes: Sequence[torch.Size],
                 lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, lr_schedule=None, momentum_buffer: Optional[torch.Tensor] = None):
        """``momentum_buffer``: an existing flat buffer to hold (an engine's own), instead of a new zeroed one."""
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.p = flat_param
        self.g = flat_grad
        self.m = torch.zeros_like(flat_param) if momentum_buffer is None else momentum_buffer
        self.shapes = [torch.Size(s) for s in param_shapes]
        group = _torch_sgd_group_defaults()
        group.update(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                     params=list(range(len(self.shapes))))
        self.param_groups = [group]
        self.step_count = 0
        self.lr_schedule = lr_schedule

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    def step(self, grad_scale: float = 1.0):
        self.step_count += 1
        g = self.param_groups[0]
        lr, lr_tab, counter = g["lr"], None, None
        if self.lr_schedule is not None:
            if self.p.is_cuda:
                lr_tab = self.lr_schedule.device_table(self.p.device)
                counter = torch.full((1,), self.step_count, dtype=torch.int32, device=self.p.device)
            else:
                lr = self.lr_schedule.rate_for(self.step_count - 1)
        sgd_flat_(self.p, self.g, self.m, self.step_count, lr, g["momentum"], g["dampening"], g["nesterov"],
                  g["weight_decay"], grad_scale=grad_scale, step_counter=counter, lr_tab=lr_tab)

    def zero_grad(self):
        self.g.zero_()

    def _views(self, flat):
        out, off = [], 0
        for s in self.shapes:
            n = s.numel()
            out.append(flat[off: off + n].view(s))
            off += n
        return out

    def state_dict(self) -> Dict:
        state = {}
        if self.step_count > 0 and self.param_groups[0]["momentum"] != 0:
            for i, mv in enumerate(self._views(self.m)):
                state[i] = {"momentum_buffer": mv.detach().to("cpu", torch.float32).clone()}
        return {"state": state, "param_groups": [dict(g) for g in self.param_groups]}

    def load_state_dict(self, sd: Dict):
        pg = sd["param_groups"][0]
        for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov"):
            if k in pg:
                self.param_groups[0][k] = pg[k]
        st = sd.get("state", {})
        loaded = False
        for i, mv in enumerate(self._views(self.m)):
            s = st.get(i, st.get(str(i)))
            if s is not None and s.get("momentum_buffer") is not None:
                mv.copy_(s["momentum_buffer"])
                loaded = True
        # (no step count in torch's SGD state: a loaded buffer means at least one step was taken - the first-step rule
        # must not overwrite it; the caller sets the true count)
        self.step_count = 1 if loaded else 0

"""Learning-rate schedules as tables of cases: the device rate table's layout and clamped read, the schedulers the
table is filled from with the plain torch loop that records their rates step by step, and the flat-Adam cases of a
launch that reads its rate from the table (fp64 reference and bounds: tests/wide_step_cases.py adam_ref, as
tests/clip_cases.py).

tests/test_lr_schedule_cpu.py checks the host side against these (trainer/lr_schedule.py, the Trainer, checkpoints,
the LearningRateMonitor); tests/test_lr_schedule_gpu.py launches the kernels (csrc/lr_table.h, csrc/adam_impl.h).

A plain module, not a conftest: the tests import it."""
import warnings

import numpy as np
import torch
from torch.optim import lr_scheduler as S

from wide_step_cases import B1, B2, EPS, Hyper, f32

# ------------------------------------------------------------------------------------------------ the table
TABLE_HEADER = 4  # words {int32 t0, int32 len, 0, 0} before lr[0] (csrc/lr_table.h)


def table_image(t0, rates):
    """The table as int32 words, written here independently of LrSchedule.table_image: header, then each rate rounded
    once to fp32."""
    img = np.zeros(TABLE_HEADER + len(rates), dtype=np.int32)
    img[0], img[1] = t0, len(rates)
    img[TABLE_HEADER:] = np.asarray(rates, dtype=np.float64).astype(np.float32).view(np.int32)
    return torch.from_numpy(img)


def table_rate(img, taken):
    """lr_for (csrc/lr_table.h) on the host: the entry for ``taken`` steps taken, index clamped to [0, len - 1]."""
    t0, n = int(img[0]), int(img[1])
    k = min(max(taken - t0, 0), n - 1)
    return float(img[TABLE_HEADER + k: TABLE_HEADER + k + 1].view(torch.float32))


# A warm-up then a decay, in a window that does not start at step 0: the steps below and past it read the clamped ends.
WINDOW_T0 = 3
WINDOW = [2.5e-4, 5e-4, 1e-3, 7e-4, 4e-4, 1e-4]
# steps taken before the launch's step -> what it is the edge of
TAKEN = {
    0: "below the window: clamps to its first entry",
    3: "the window's first entry",
    5: "the peak, inside the window",
    8: "the window's last entry",
    20: "past the window: clamps to its last entry",
}


def window_image():
    return table_image(WINDOW_T0, WINDOW)


# ------------------------------------------------------------------------------------------------ schedulers
BASE_LR = 0.1
PLATEAU_METRICS = [1.0 + 0.1 * e for e in range(12)]  # the monitored metric of epoch e: never improves on the first


class HalveEvery:
    """A user-written multiplier (a callable object: LambdaLR keeps its __dict__ in the state dict)."""

    def __init__(self, every):
        self.every = every

    def __call__(self, k):
        return 0.5 ** (k // self.every)


def _sequential(opt):
    warm = S.LinearLR(opt, start_factor=0.1, total_iters=4)
    cos = S.CosineAnnealingLR(opt, T_max=9, eta_min=1e-3)
    return S.SequentialLR(opt, [warm, cos], milestones=[4])


# name -> scheduler factory over an optimizer
SCHEDULERS = {
    "StepLR": lambda opt: S.StepLR(opt, step_size=2, gamma=0.5),
    "ExponentialLR": lambda opt: S.ExponentialLR(opt, gamma=0.9),
    "CosineAnnealingLR": lambda opt: S.CosineAnnealingLR(opt, T_max=7, eta_min=1e-4),
    "SequentialLR": _sequential,
    "LambdaLR": lambda opt: S.LambdaLR(opt, HalveEvery(3)),
    "ReduceLROnPlateau": lambda opt: S.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=1),
}
INTERVALS = [("step", 1), ("step", 3), ("epoch", 1), ("epoch", 3)]


def is_plateau(sched):
    return isinstance(sched, S.ReduceLROnPlateau)


def new_optimizer(lr=BASE_LR):
    return torch.optim.Adam([torch.zeros(3, requires_grad=True)], lr=lr)


def torch_rates(name, interval, frequency, n_steps, epochs, metrics=PLATEAU_METRICS):
    """[epoch][step] rates of a plain torch loop: optimizer.step() per batch; scheduler.step() after batch b of the
    epoch when (b + 1) % frequency == 0 (interval "step") or after epoch e when (e + 1) % frequency == 0 ("epoch",
    ReduceLROnPlateau on metrics[e]) - Lightning's rules."""
    opt = new_optimizer()
    sched = SCHEDULERS[name](opt)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for e in range(epochs):
            rates = []
            for b in range(n_steps):
                rates.append(float(opt.param_groups[0]["lr"]))
                opt.step()
                if interval == "step" and (b + 1) % frequency == 0:
                    sched.step()
            out.append(rates)
            if interval == "epoch" and (e + 1) % frequency == 0:
                sched.step(metrics[e]) if is_plateau(sched) else sched.step()
    return out


# ------------------------------------------------------------------------------------------------ flat Adam
# sizes: the float4 tail, and one past a whole grid pass of the Adam launch (2048 workgroups of 256 float4s)
ADAM_N_TAIL = 1027
ADAM_N_TWO_PASSES = 4 * 2048 * 256 + 4 * 300 + 3
# (name, Hyper without its rate): plain Adam, and AdamW - decoupled decay's term is lr * wd * p, so its rate is checked
ADAM_HYPERS = {
    "adam": Hyper(None, B1, B2, EPS, 0.0, 1.0, 0),
    "adam_scaled_l2": Hyper(None, B1, B2, EPS, 0.05, 0.125, 0),
    "adamw": Hyper(None, B1, B2, EPS, 0.05, 1.0, 1),
}
SCALAR_LR = 0.5  # the scalar a table launch is also given: a launch that ignores its table lands far outside the bound


def hyper_at(hp, taken, img=None):
    """``hp`` with the rate the table holds for ``taken`` steps taken (an fp32 value: what a scalar launch is given)."""
    return hp._replace(lr=f32(table_rate(window_image() if img is None else img, taken)))


# ------------------------------------------------------------------------------------------------ persistent trainers
# One K-step launch of a small-MLP trainer against K one-step launches of the same kernel.  The launches start after
# FAMILY_START steps; the window starts two steps later and ends two steps before the launch does, so the first and
# the last steps read the clamped ends.
FAMILY_START = 2
FAMILY_LR = 0.01


def family_window(steps):
    """(t0, rates) for a launch of ``steps`` steps: a linear warm-up over the first third, then a 3 % decay per step."""
    n = steps - 4
    warm = max(1, n // 3)
    rates = [FAMILY_LR * (k + 1) / warm if k < warm else FAMILY_LR * 0.97 ** (k - warm + 1) for k in range(n)]
    return FAMILY_START + 2, rates


# name -> (environment, dims, batch, bmax of the plan, steps, rows missing in the last batch, the trainer that must run,
#          single-wave kernel asked for through its phase-stamp buffer)
NOENV = {"DCT_B5_SCHED": None, "DCT_MLP_KERNEL": None, "DCT_MLP_BLOCK": None}
FAMILIES = {
    "block5": (NOENV, [5, 128, 128, 2], 4, 4, 70, 1, "block5", False),  # 70 steps cross the 64-step lane refill
    "block5_sched0": (dict(NOENV, DCT_B5_SCHED="0"), [5, 128, 128, 2], 4, 4, 70, 1, "block5", False),
    "block5_b8": (NOENV, [5, 128, 128, 2], 8, 16, 70, 1, "block5_b8", False),
    "block5_b8_forced_b4": (dict(NOENV, DCT_MLP_BLOCK="8"), [5, 128, 128, 2], 4, 4, 70, 1, "block5_b8", False),
    "block3": (dict(NOENV, DCT_MLP_BLOCK="3"), [7, 128, 128, 2], 4, 4, 7, 1, "block3", False),
    "wave_rows": (NOENV, [5, 64, 2], 4, 4, 7, 1, "wave_rows", False),
    "wave_single": (NOENV, [5, 64, 2], 4, 4, 7, 1, "wave_single", True),
    "lds": (dict(NOENV, DCT_MLP_KERNEL="lds"), [5, 64, 2], 4, 4, 7, 1, "lds", False),
    "tile": (NOENV, [5, 64, 2], 33, 1024, 7, 1, "tile", False),  # two tiles of 32 rows
}

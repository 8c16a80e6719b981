"""Gradient clipping in the batch-tiled MLP trainer, the parts that need no device: the selector's refusal of a clipped
launch on every other plan, MlpPlan.trainer(clipped=True), and Trainer(engine="tile") routing with stand-in engines."""
import types

import pytest
import torch

import dct_amd  # noqa: F401
import dct_amd.trainer.trainer as trainer_mod
from dct_amd.models.mlp import MLPClassifier
from dct_amd.ops._native import native
from dct_amd.trainer import Trainer


@pytest.mark.parametrize("dims,bmax", [([5, 64, 2], 4), ([5, 128, 128, 2], 4), ([5, 128, 128, 2], 16), ([20, 96, 3], 16)])
def test_a_clipped_launch_is_refused_on_wave_block_and_lds_plans(dims, bmax):
    plan = native().MlpPlan(dims, bmax)
    assert plan.trainer(bmax) not in ("tile", "none") and plan.trainer(bmax, clipped=True) == "none"
    assert plan.trainer(bmax, mode=1, clipped=True) == plan.trainer(bmax, mode=1)  # grad mode ignores clipping
    for kind in (1, 2):  # (refused before any pointer is touched: none is bound)
        with pytest.raises(ValueError, match=r"gradient clipping needs the batch-tiled trainer's plan \(bmax 1024\)"):
            plan.train(0, 0, 0, 0, 0, dims[0], 0, 0, 64, bmax, 1, 0, 0.01, 0.9, 0.999, 1e-8, 0.0, 0.0, 0, 0, 0, 0, 0,
                       0, 0, clip_kind=kind, clip_val=1.0)


def test_the_tile_plan_takes_clipped_launches():
    plan = native().MlpPlan([5, 64, 2], 1024)
    for b in (1, 16, 17, 1024):
        assert plan.trainer(b, clipped=True) == "tile"
        assert plan.trainer(b, clipped=True, accumulate=3, optimizer="sgd", weighted=True) == "tile"
    assert plan.trainer(1025, clipped=True) == "none"
    assert plan.trainer(1024, clipped=True, accumulate=9) == "none"  # 9 * 32 slots: over the cap
    assert native().MlpPlan([5, 300, 2], 16).trainer(4, clipped=True) == "none"
    assert native().mlp_tile_clip_ws_floats([5, 64, 2]) == 516 + 4 + 4  # gf[P + 1] | part[3] | stats, each padded to 4
    assert native().mlp_tile_clip_ws_floats([5, 300, 2]) == 0


@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("batch", [4, 64])
def test_engine_tile_takes_a_clipped_model_to_the_fused_engine(monkeypatch, batch, algorithm):
    """The class _make_engine picks with every engine replaced by a recording stand-in, as test_grad_clip_cpu.py."""
    clip = dict(gradient_clip_val=0.5, gradient_clip_algorithm=algorithm)

    def routed(engine, fused_ok=True, env=None, **kw):
        for n in ("FusedMLPEngine", "GraphMLPEngine", "AutogradEngine"):
            fake = type(n, (), dict(__init__=lambda self, *a, **k: setattr(self, "kw", k),
                                    applicable=staticmethod(lambda *a, ok=(fused_ok or n[0] != "F"), **k: ok)))
            monkeypatch.setattr(trainer_mod, n, fake)
        monkeypatch.setenv("DCT_ENGINE", env) if env else monkeypatch.delenv("DCT_ENGINE", raising=False)
        t = Trainer(accelerator="cpu", engine=engine, verbose=False, **kw)
        t.ctx = types.SimpleNamespace(device=torch.device("cpu"))
        e = t._make_engine(MLPClassifier(5, (64,), dropout=0.2), batch, 0)
        return type(e).__name__, e.kw

    for engine, env in (("tile", None), ("auto", "tile")):
        name, kw = routed(engine, env=env, **clip)
        assert name == "FusedMLPEngine" and {k: kw[k] for k in clip} == clip and kw["tile_plan"] is True
    name, kw = routed("tile", accumulate_grad_batches=3, **clip)
    assert name == "FusedMLPEngine" and kw["accumulate_grad_batches"] == 3
    name, kw = routed("tile")  # unclipped: still the tile plan
    assert name == "FusedMLPEngine" and kw["gradient_clip_val"] is None and kw["tile_plan"] is True
    with pytest.raises(RuntimeError, match="engine='tile' requested"):
        routed("tile", fused_ok=False, **clip)
    assert routed("auto", **clip)[0] == "GraphMLPEngine"  # auto routes clipped models as before

"""The wide bf16 inference kernel (csrc/mlp_wide_infer.hip) against a plain fp64 forward with the kernel's rounding
points: weights, the (normalised) input and every hidden activation rounded to bf16, biases fp32.

The bound is LIMIT times the error of torch's own bf16 forward (F.linear on bf16 tensors, the same rounding points, on
the GPU) against the same reference, taken per case as the largest error over the case's 197 rows.  Measured on an
MI355X, kernel error / torch error, largest over the four row counts (logits, probabilities):
    32x128x2 (0.000, 0.000), 64x256x128x3 (0.122, 0.051), 256x1024x1024x1024x2 (0.453, 0.249), 96x384x8 (0.013, 0.011)
LIMIT is the power of two at or above 4 times the largest ratio, 4 * 0.453 = 1.81 -> 2 (profiles/wide_infer_cost.log)."""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

import infer_cases as ic

import dct_amd  # noqa: F401
from dct_amd.data.dataset import TensorPairDataset
from dct_amd.models.mlp import MLPClassifier
from dct_amd.ops._native import native, ptr, stream_handle
from dct_amd.ops.fused_mlp import FusedMLPKernel, weighted_infer_stats
from dct_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
LIMIT = 2.0
BM = 64  # rows of the kernel's tile
ROWS = (1, BM, BM + 1, 3 * BM + 5)
N = ROWS[-1]
# one k-step group and 16 columns per wave / shrinking widths (stale image columns) / full register slab and image /
# C = 8 and K no power of two; the options spread over them
CASES = {
    "32x128x2": dict(dims=[32, 128, 2], act="relu", loss="ce", seed=3),
    "64x256x128x3": dict(dims=[64, 256, 128, 3], act="gelu", loss="mse", dup=True, seed=18),
    "256x1024x1024x1024x2": dict(dims=[256, 1024, 1024, 1024, 2], act="relu", loss="ce", norm=True, seed=11),
    "96x384x8": dict(dims=[96, 384, 8], act="gelu", loss="ce", cw=True, smooth=0.1, seed=2),
}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """fp32 / integer inputs on the CPU: layers [(W, b)], flat p, X [N, D0], Y, idx (with duplicates) or None,
    norm = (mean, std with its one zero replaced by 1) or None, class weights or None."""
    c = CASES[case]
    dims, g = c["dims"], torch.Generator().manual_seed(c["seed"])
    layers = [(torch.randn(o, i, generator=g) * (2.0 / i) ** 0.5, torch.randn(o, generator=g) * 0.1)
              for i, o in zip(dims[:-1], dims[1:])]
    # rows scatter around one prototype per class, so that most top-2 logit gaps are wide against the bf16 bound
    Y = torch.randint(0, dims[-1], (N,), generator=g, dtype=torch.int32)
    X = torch.randn(dims[-1], dims[0], generator=g)[Y.long()] + 0.3 * torch.randn(N, dims[0], generator=g)
    norm = None
    if c.get("norm"):
        mean, std = torch.randn(dims[0], generator=g), torch.rand(dims[0], generator=g) + 0.5
        std[3] = 0.0
        X = X * std + mean  # (column 3 is constant)
        norm = (mean, torch.where(std == 0, torch.ones_like(std), std))
    idx = torch.randint(0, N, (N,), generator=g, dtype=torch.int32) if c.get("dup") else None
    if idx is not None:
        idx[1] = idx[0]
    return dict(layers=layers, p=torch.cat([t.reshape(-1) for Wb in layers for t in Wb]), X=X, Y=Y, idx=idx, norm=norm,
                cw=torch.rand(dims[-1], generator=g) + 0.5 if c.get("cw") else None)


def forward(case, dtype, device="cpu"):
    """Logits of the N rows the launches visit.  torch.float64: the reference; torch.bfloat16: torch's own bf16 forward."""
    c, d = CASES[case], inputs(case)
    h = d["X"] if d["idx"] is None else d["X"][d["idx"].long()]
    if d["norm"] is not None:
        h = (h - d["norm"][0]) / d["norm"][1]  # fp32, as in the gather
    h = h.to(device).to(torch.bfloat16).to(dtype)
    for l, (W, b) in enumerate(d["layers"]):
        h = F.linear(h, W.to(device).to(torch.bfloat16).to(dtype), b.to(device).to(dtype))
        if l < len(d["layers"]) - 1:
            h = (F.relu(h) if c["act"] == "relu" else F.gelu(h)).to(torch.bfloat16).to(dtype)
    return h.double().cpu()


@functools.lru_cache(maxsize=None)
def reference(case):
    """fp64 logits, probabilities, argmax, labels, per-row loss (the weighted numerator with class weights / smoothing)
    and its Lipschitz constant in the logits' max norm."""
    c, d = CASES[case], inputs(case)
    z, C = forward(case, torch.float64), c["dims"][-1]
    y = (d["Y"] if d["idx"] is None else d["Y"][d["idx"].long()]).long()
    onehot = F.one_hot(y, C).double()
    if c["loss"] == "mse":
        row_loss, lip = ((z - onehot) ** 2).mean(1), 2 * (z - onehot).abs().mean(1)
    else:
        w, eps = (torch.ones(C) if d["cw"] is None else d["cw"]).double(), c.get("smooth", 0.0)
        t = (1 - eps) * w[y][:, None] * onehot + eps / C * w[None, :]
        row_loss, lip = -(t * torch.log_softmax(z, 1)).sum(1), 2 * t.sum(1)
    top2 = z.topk(2, dim=1).values
    return dict(z=z, p=torch.softmax(z, 1), pred=z.argmax(1), y=y, row_loss=row_loss, lip=lip, gap=top2[:, 0] - top2[:, 1])


def torch_error(case, device):
    """(logit error, probability error) of torch's bf16 forward against the reference, the largest over the N rows."""
    ref, zt = reference(case), forward(case, torch.bfloat16, device)
    return float((zt - ref["z"]).abs().max()), float((torch.softmax(zt, 1) - ref["p"]).abs().max())


@functools.lru_cache(maxsize=None)
def _torch_error_gpu(case):
    return torch_error(case, "cuda")


def _launch(case, n, cuda, grid=None):
    c, d = CASES[case], inputs(case)
    C = c["dims"][-1]
    kern = FusedMLPKernel(c["dims"], bmax=4)
    out = dict(logits=torch.empty(n, C, device=cuda), probs=torch.empty(n, C, device=cuda),
               pred=torch.empty(n, dtype=torch.int32, device=cuda), stats=torch.zeros(2 + C * C, dtype=torch.int64, device=cuda))
    kern.wide_infer(d["p"].to(cuda), d["X"].to(cuda), n, idx=None if d["idx"] is None else d["idx"].to(cuda),
                    Y=d["Y"].to(cuda), loss=c["loss"], logits_out=out["logits"], probs_out=out["probs"],
                    pred_out=out["pred"], stats_out=out["stats"], grid=grid, activation=c["act"],
                    norm=None if d["norm"] is None else tuple(t.to(cuda) for t in d["norm"]),
                    class_weight=None if d["cw"] is None else d["cw"].to(cuda), label_smoothing=c.get("smooth", 0.0))
    out = {k: v.cpu() for k, v in out.items()}
    out["kernel"] = kern
    return out


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("case", CASES)
def test_kernel_matches_fp64_within_limit_times_torchs_bf16_error(case, n, cuda):
    ref, got, C = reference(case), _launch(case, n, cuda), CASES[case]["dims"][-1]
    tz, tp = _torch_error_gpu(case)
    kz = float((got["logits"].double() - ref["z"][:n]).abs().max())
    kp = float((got["probs"].double() - ref["p"][:n]).abs().max())
    print(f"{case} n={n}: logits kernel {kz:.3e} torch {tz:.3e} ratio {kz / tz:.3f}; "
          f"probs kernel {kp:.3e} torch {tp:.3e} ratio {kp / tp:.3f}")
    assert kz <= LIMIT * tz and kp <= LIMIT * tp
    assert torch.equal(got["pred"].long(), got["logits"].argmax(1))  # lowest index on ties included
    # the loss sum: a row's loss moves by at most lip * b + b^2 (the MSE's second order) for logits moved by b, the
    # logit bound; fp32 exp / log / sums add 2^-20 relative
    loss_sum, correct, conf = got["kernel"].infer_stats(got["stats"])
    b = LIMIT * tz
    tol = float((ref["lip"][:n] * b + b * b + 2.0 ** -20 * (1 + ref["z"][:n].abs().max(1).values)).sum())
    print(f"{case} n={n}: loss sum err {abs(loss_sum - float(ref['row_loss'][:n].sum())):.3e} tol {tol:.3e}")
    assert abs(loss_sum - float(ref["row_loss"][:n].sum())) <= tol
    # counts: exact on the rows whose fp64 top-2 gap the bound decides, the launch's own argmax on the others
    amb = ref["gap"][:n] < 2 * LIMIT * tz
    assert int(amb.sum()) <= ic.MAX_AMBIGUOUS * n
    pred = torch.where(amb, got["pred"].long(), ref["pred"][:n])
    assert correct == int((pred == ref["y"][:n]).sum()) and torch.equal(conf, ic.confusion(ref["y"][:n], pred, C))
    if CASES[case].get("cw"):  # the weighted mean divides by W from the confusion matrix's row sums
        mean, _, _ = weighted_infer_stats(loss_sum, correct, conf, inputs(case)["cw"])
        W = float(inputs(case)["cw"].double()[ref["y"][:n]].sum())
        assert abs(mean - float(ref["row_loss"][:n].sum()) / W) <= tol / W


@pytest.mark.parametrize("case", CASES)
def test_outputs_and_statistics_are_bit_identical_across_grids(case, cuda):
    """grid = 1 and 2 make a workgroup walk several slots; every output has the default grid's bits."""
    runs = [_launch(case, N, cuda, grid=g) for g in (None, 1, 2)]
    for r in runs[1:]:
        assert all(torch.equal(r[k], runs[0][k]) for k in ("stats", "logits", "probs", "pred"))


@pytest.mark.parametrize("dims", [[8, 1024, 2], [256, 1000, 2], [256, 1024, 9], [32, 128, 128, 128, 128, 2]])
def test_launcher_refuses_other_shapes_and_writes_nothing(dims, cuda):
    C, n = dims[-1], 8
    p = torch.zeros(ic.num_params(dims), device=cuda)
    X, Y = torch.zeros(n, dims[0], device=cuda), torch.zeros(n, dtype=torch.int32, device=cuda)
    logits = torch.full((n, C), 12345.0, device=cuda)
    ws, stats = (torch.full((2 + C * C,), -1, dtype=torch.int64, device=cuda) for _ in range(2))
    assert native().mlp_wide_infer_ws_bytes(dims, n) == 0
    with pytest.raises(RuntimeError, match="invalid"):
        native().mlp_wide_infer(dims, ptr(p), ptr(p.to(torch.bfloat16)), ptr(X), X.stride(0), 0, ptr(Y), n, 0, 0, 0,
                                ptr(logits), 0, 0, ptr(ws), ws.numel() * 8, ptr(stats), 0, stream_handle())
    torch.cuda.synchronize()
    assert bool((logits == 12345.0).all()) and bool((ws == -1).all()) and bool((stats == -1).all())
    with pytest.raises(ValueError):
        FusedMLPKernel(dims, bmax=4).wide_infer(p, X, n, logits_out=logits)


def test_trainer_test_and_predict_take_the_wide_kernel(cuda):
    """Fit-free: Trainer.test / predict of a 64-256-256-2 model on 300 rows give the direct launch's numbers."""
    dims, n, g = [64, 256, 256, 2], 300, torch.Generator().manual_seed(11)
    torch.manual_seed(5)
    model = MLPClassifier(64, hidden=(256, 256), dropout=0.0)
    x, y = torch.randn(n, 64, generator=g), torch.randint(0, 2, (n,), generator=g)
    loader = DataLoader(TensorPairDataset(x, y), batch_size=128)
    p = torch.cat([t.detach().reshape(-1) for lin in model.linear_layers() for t in (lin.weight, lin.bias)]).to(cuda)
    kern, logits = FusedMLPKernel(dims, bmax=4), torch.empty(n, 2, device=cuda)
    stats = torch.zeros(6, dtype=torch.int64, device=cuda)
    kern.wide_infer(p, x.to(cuda), n, Y=y.to(cuda, torch.int32), logits_out=logits, stats_out=stats)
    loss_sum, correct, conf = kern.infer_stats(stats)
    t = Trainer(accelerator="gpu", logger=None, verbose=False)
    out = t.test(model, loader)[0]
    assert out == {"test_loss": loss_sum / n, "test_acc": correct / n}
    assert torch.equal(t.last_confusion_matrix, conf) and int(conf.sum()) == n
    preds = t.predict(model, loader)
    assert [tuple(q.shape) for q in preds] == [(128, 2), (128, 2), (44, 2)]
    assert torch.equal(torch.cat(preds), logits)

#!/usr/bin/env python
"""One sha256 per case of what the batch-tiled trainer (csrc/mlp_tile.hip) and the batch-tiled inference kernel
(csrc/mlp_infer.hip) compute from seeded inputs: two builds of the extension that print the same listing compute the
same bits (run it once per build, tools/so_ab.sh style, and diff the listings).

  trainer    dims 5-64-2, 7-48-32-3, 5-128-128-2, 32-128-128-4; batch 33 and 165 (2 and 6 tiles, the last one partial);
             CE and MSE; dropout 0 and 0.2.  Three Adam steps, then one grad-mode launch on the updated parameters.
             Hashed: p, m, v, the three losses, grad_out (gradients + loss).
  inference  the same dims; n = 33 and 165; over X itself, and through a repeating index list with (x - mean) / std in
             the gather.  Hashed: logits, probabilities, predictions, statistics.

The tool fails without a GPU.

    python tools/tile_bits.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DIMS = ([5, 64, 2], [7, 48, 32, 3], [5, 128, 128, 2], [32, 128, 128, 4])
ROWS = (33, 165)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def problem(dims, n, dev):
    import torch

    from dct_amd.ops.fused_mlp import mlp_num_params

    g = torch.Generator().manual_seed(1000 * sum(dims) + n)
    N = 3 * n + 37
    p = (torch.rand(mlp_num_params(dims), generator=g) * 2 - 1) * 0.3
    X = torch.randn(N, dims[0], generator=g)
    Y = torch.randint(0, dims[-1], (N,), generator=g, dtype=torch.int32)
    idx = torch.randint(0, N, (3 * n,), generator=g, dtype=torch.int32)  # repeats rows
    return p.to(dev), X.to(dev), Y.to(dev), idx.to(dev)


def train_case(dims, B, loss, dropout, dev):
    import torch

    from dct_amd.ops.fused_mlp import FusedMLPKernel

    p, X, Y, idx = problem(dims, B, dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(3, device=dev)
    grad = torch.zeros(p.numel() + 1, device=dev)
    k = FusedMLPKernel(dims, bmax=1024)
    assert k.plan.trainer(B) == "tile"
    kw = dict(lr=0.01, weight_decay=0.01, dropout=dropout, seed=11, loss=loss)
    k.train(p, m, v, X, Y, idx, n_items=3 * B - 4, batch=B, steps=3, t0=2, step_base=5, loss_out=losses, **kw)
    k.train(p, None, None, X, Y, idx, n_items=B, batch=B, steps=1, t0=0, step_base=8, grad_out=grad, **kw)
    torch.cuda.synchronize()
    return digest(p, m, v, losses, grad)


def infer_case(dims, n, gather, dev):
    import torch

    from dct_amd.ops.fused_mlp import FusedMLPKernel

    p, X, Y, idx = problem(dims, n, dev)
    C = dims[-1]
    logits, probs = torch.zeros(n, C, device=dev), torch.zeros(n, C, device=dev)
    pred = torch.zeros(n, dtype=torch.int32, device=dev)
    stats = torch.zeros(2 + C * C, dtype=torch.int64, device=dev)
    norm = (X.mean(0).contiguous(), X.std(0).contiguous()) if gather else None
    FusedMLPKernel(dims, bmax=1024).infer(p, X, n, idx=idx if gather else None, Y=Y, logits_out=logits, probs_out=probs,
                                          pred_out=pred, stats_out=stats, norm=norm)
    torch.cuda.synchronize()
    return digest(logits, probs, pred, stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import dct_amd  # noqa: F401

    if not torch.cuda.is_available():
        raise SystemExit("tile_bits.py needs a GPU")
    dev = torch.device("cuda", 0)
    lines = []
    for dims in DIMS:
        name = "-".join(map(str, dims))
        for n in ROWS:
            for loss, dropout in (("ce", 0.0), ("ce", 0.2), ("mse", 0.0), ("mse", 0.2)):
                lines.append(f"train {name} B={n} {loss} dropout={dropout}: " + train_case(dims, n, loss, dropout, dev))
            for gather in (False, True):
                lines.append(f"infer {name} n={n} {'idx+norm' if gather else 'plain'}: " + infer_case(dims, n, gather, dev))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

"""Batch scoring job: score a held-out or fresh table with a checkpoint, through ``Trainer.predict``.

    python jobs/score_batch.py --ckpt model.ckpt --input /data/processed --output scores.parquet
    python jobs/score_batch.py --ckpt model.ckpt --synthetic-rows 1000 --output scores.npy --raw

The model is rebuilt from the checkpoint's ``hyper_parameters`` (MLP family only).  ``--input`` is a directory with
``data.parquet``: the ``*_norm`` feature columns, or with ``--raw`` the raw columns ``norm_stats.json`` (next to the
checkpoint, as the packaged ``score.py`` reads it) names, normalised as ``(x - mean) / std`` with a zero std replaced
by 1.  The output holds one row per input row: the class probabilities and the predicted class - ``.parquet``
(``prob_<c>`` columns + ``prediction``) through pyarrow when it is importable, otherwise ``.npy`` (fp32
``[n, C + 1]``, the prediction in the last column).  All logic lives in the package; this file handles arguments.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dct_amd  # noqa: E402,F401
from dct_amd.ckpt.lightning_io import load_checkpoint  # noqa: E402
from dct_amd.models.mlp import MLPClassifier  # noqa: E402
from dct_amd.trainer import Trainer  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--ckpt", required=True, help="checkpoint file (Lightning layout)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", help="directory with data.parquet")
    src.add_argument("--synthetic-rows", type=int, default=0, help="score N synthetic weather rows instead")
    p.add_argument("--output", required=True, help=".parquet (needs pyarrow) or .npy")
    p.add_argument("--raw", action="store_true", help="inputs are raw: normalise with norm_stats.json next to --ckpt")
    p.add_argument("--accelerator", default="auto")
    p.add_argument("--batch-size", type=int, default=4096)
    return p.parse_args(argv)


def model_from_checkpoint(path: str) -> MLPClassifier:
    hp = dict(load_checkpoint(path).get("hyper_parameters") or {})
    if "input_dim" not in hp:
        raise ValueError(f"{path}: not an MLP-family checkpoint (hyper_parameters {sorted(hp)}): "
                         "score_batch scores the MLP family only")
    kw = {k: hp[k] for k in ("hidden", "num_classes", "dropout", "loss", "class_weight", "label_smoothing") if k in hp}
    return MLPClassifier(int(hp["input_dim"]), **kw)


def norm_stats(ckpt: str):
    """(columns, mean, std) of norm_stats.json next to the checkpoint; a std of 0 (or null) becomes 1."""
    import torch

    sp = os.path.join(os.path.dirname(os.path.abspath(ckpt)), "norm_stats.json")
    if not os.path.exists(sp):
        raise ValueError("raw inputs need norm_stats.json next to the checkpoint")
    with open(sp) as f:
        st = json.load(f)
    cols = list(st)
    mean = torch.tensor([float(st[c]["mean"]) for c in cols], dtype=torch.float32)
    std = torch.tensor([float(st[c]["std"]) if st[c]["std"] not in (None, 0) else 1.0 for c in cols],
                       dtype=torch.float32)
    return cols, mean, std


def load_rows(a, norm=None):
    """fp32 [n, D] features: the parquet's columns or synthetic rows (raw-scale under --raw)."""
    import torch

    if a.synthetic_rows > 0:
        from dct_amd.data.synthetic import weather_tensors

        x, _ = weather_tensors(a.synthetic_rows, seed=0)
        return x * norm[2] + norm[1] if norm is not None else x
    if norm is not None:
        import pandas as pd

        df = pd.read_parquet(os.path.join(a.input, "data.parquet"))
        return torch.tensor(df[norm[0]].to_numpy(), dtype=torch.float32)
    from dct_amd.data.dataset import WeatherDataset

    return WeatherDataset(a.input, verbose=False).features


def write_scores(path: str, probs, pred) -> str:
    try:
        import pyarrow as pa
        import pyarrow.parquet as pq
    except ImportError:
        pa = None
    if path.endswith(".parquet") and pa is not None:
        cols = {f"prob_{c}": probs[:, c].numpy() for c in range(probs.shape[1])}
        cols["prediction"] = pred.numpy()
        pq.write_table(pa.table(cols), path)
        return path
    import numpy as np
    import torch

    path = os.path.splitext(path)[0] + ".npy"
    np.save(path, torch.cat([probs, pred[:, None].to(probs.dtype)], 1).numpy())
    return path


def main(argv=None) -> int:
    import torch
    from torch.utils.data import DataLoader, TensorDataset

    a = parse_args(argv)
    model = model_from_checkpoint(a.ckpt)
    norm = norm_stats(a.ckpt) if a.raw else None
    x = load_rows(a, norm)
    trainer = Trainer(accelerator=a.accelerator, logger=None, verbose=False)
    if norm is not None:
        trainer.input_norm = (norm[1], norm[2])
    batches = trainer.predict(model, DataLoader(TensorDataset(x), batch_size=a.batch_size), ckpt_path=a.ckpt)
    logits = torch.cat([b.float().cpu() for b in batches])
    out = write_scores(a.output, torch.softmax(logits, 1), logits.argmax(1))
    print(f"scored {len(logits)} rows -> {out}")
    trainer.teardown()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Worker for tests/test_lr_schedule_gpu.py: two data-parallel 'ranks' as concurrent persistent launches on two
streams of one GPU (peers = raw pointers, as tests/test_xg_block5_gpu._in_process_run), training with the in-kernel
gradient exchange while every step takes its rate from a device rate table.  Run in a fresh process:

    python lr_xg_worker.py OUT.json DIMS(comma separated) STEPS B T0 RATE[,RATE..]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import dct_amd  # noqa: E402,F401
import lr_cases as L  # noqa: E402
from dct_amd.data.sampler import distributed_indices  # noqa: E402
from dct_amd.data.synthetic import weather_tensors  # noqa: E402
from dct_amd.ops._native import native  # noqa: E402
from dct_amd.ops.fused_mlp import FusedMLPKernel  # noqa: E402

W, ROWS = 2, 3000


def net(dims, seed=1):
    torch.manual_seed(seed)
    layers = []
    for i in range(len(dims) - 1):
        layers += [torch.nn.Linear(dims[i], dims[i + 1])] + ([torch.nn.ReLU()] if i < len(dims) - 2 else [])
    return torch.nn.Sequential(*layers)


def problem():
    X, Y = weather_tensors(ROWS, seed=5)
    return X, Y, [distributed_indices(ROWS, W, r, shuffle=True, seed=42, epoch=0) for r in range(W)]


def main():
    out_path, dims, steps, B, t0 = (sys.argv[1], [int(d) for d in sys.argv[2].split(",")], int(sys.argv[3]),
                                    int(sys.argv[4]), int(sys.argv[5]))
    rates = [float(r) for r in sys.argv[6].split(",")]
    nat = native()
    cuda = torch.device("cuda", 0)
    kern = FusedMLPKernel(dims, bmax=4)
    assert kern.xg_supported(B, W)
    xs = [nat.PeerExchange(W, r, kern.xg_buffer_bytes(W, B)) for r in range(W)]
    for x in xs:
        x.set_peers([y.recv for y in xs])
    X, Y, shards = problem()
    p0 = torch.cat([t.detach().reshape(-1) for t in net(dims).state_dict().values()])
    ps = [p0.clone().to(cuda) for _ in range(W)]
    ms = [torch.zeros_like(ps[0]) for _ in range(W)]
    vs = [torch.zeros_like(ps[0]) for _ in range(W)]
    losses = [torch.zeros(steps, device=cuda) for _ in range(W)]
    scs = [torch.zeros(1, dtype=torch.int32, device=cuda) for _ in range(W)]
    tab = L.table_image(t0, rates).to(cuda).view(torch.float32)
    Xd, Yd = X.to(cuda), Y.to(cuda, torch.int32)
    idx = [s.to(cuda, torch.int32) for s in shards]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(cuda) for _ in range(W)]
    for r in range(W):  # (the scalar rate is far from the table's: a launch that ignored its table would show)
        kern.train(ps[r], ms[r], vs[r], Xd, Yd, idx[r], n_items=idx[r].numel(), batch=B, steps=steps, t0=0, lr=0.5,
                   loss_out=losses[r], step_counter=scs[r], xg=xs[r], xg_timeout_s=5.0, stream=streams[r].cuda_stream,
                   lr_tab=tab)
    torch.cuda.synchronize()
    json.dump({"trainer": kern.plan.trainer(B, mode=0, steps=steps, world=W), "status": [x.read_status() for x in xs],
               "steps": [int(sc.item()) for sc in scs], "params": [p.cpu().tolist() for p in ps],
               "m": [m.cpu().tolist() for m in ms], "v": [v.cpu().tolist() for v in vs],
               "losses": [l.cpu().tolist() for l in losses]}, open(out_path, "w"))


if __name__ == "__main__":
    main()

"""The batch-tiled inference kernel (csrc/mlp_infer.hip) against the fp64 reference of tests/infer_cases.py: every
output inside the derived bound, integer statistics exact, statistics bit-identical across grids and runs."""
import pytest
import torch

import infer_cases as ic

import dct_amd  # noqa: F401
from dct_amd.ops._native import native, ptr, stream_handle
from dct_amd.ops.fused_mlp import FusedMLPKernel

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in ic.CASES]
POISON = 12345.0


def _launch(case, cuda, grid="case", with_y=True, outs=("logits", "probs", "pred"), norm="case"):
    """One launch of a case; returns dict(logits, probs, pred on the CPU or None, stats tensor on the device)."""
    c, d = ic.BY_NAME[case], ic.inputs(case)
    n, C = c["n"], c["dims"][-1]
    kern = FusedMLPKernel(c["dims"], bmax=1024)
    X = d["table"].to(cuda)[:, : c["dims"][0]]  # a view of the wider table: row stride D0 + 3
    assert X.stride(0) == d["X"].stride(0) > c["dims"][0]
    bufs = dict(logits=torch.full((n, C), POISON, device=cuda), probs=torch.full((n, C), POISON, device=cuda),
                pred=torch.full((n,), -7, dtype=torch.int32, device=cuda))
    stats = torch.full((2 + C * C,), -1, dtype=torch.int64, device=cuda)
    nm = d["norm"] if norm == "case" else norm
    kern.infer(d["p"].to(cuda), X, n, idx=None if d["idx"] is None else d["idx"].to(cuda),
               Y=d["Y"].to(cuda) if with_y else None, loss=c["loss"],
               logits_out=bufs["logits"] if "logits" in outs else None,
               probs_out=bufs["probs"] if "probs" in outs else None, pred_out=bufs["pred"] if "pred" in outs else None,
               stats_out=stats, norm=None if nm is None else tuple(t.to(cuda) for t in nm),
               grid=c["grid"] if grid == "case" else grid)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in bufs.items()}
    out["stats"] = stats
    out["kernel"] = kern
    return out


@pytest.mark.parametrize("case", NAMES)
def test_case_matches_fp64_inside_the_derived_bound(case, cuda):
    c, ref = ic.BY_NAME[case], ic.reference(case)
    n, C = c["n"], c["dims"][-1]
    got = _launch(case, cuda)
    err_z = (got["logits"].double() - ref["logits"]).abs()
    err_p = (got["probs"].double() - ref["probs"]).abs()
    print(f"{case}: logits err/bound {float((err_z / ref['bound_z']).max()):.3f}, "
          f"probs err/bound {float((err_p / ref['bound_p']).max()):.3f}, ambiguous {int(ref['ambiguous'].sum())}")
    assert bool((err_z <= ref["bound_z"]).all())
    assert bool(torch.isfinite(got["probs"]).all()) and bool((err_p <= ref["bound_p"]).all())
    assert float((got["probs"].double().sum(1) - 1).abs().max()) <= 4 * 2.0 ** -23  # <= 4 roundings of a sum near 1
    clear = ~ref["ambiguous"]
    assert int(ref["ambiguous"].sum()) <= ic.MAX_AMBIGUOUS * n
    assert torch.equal(got["pred"].long()[clear], ref["pred"][clear])
    assert torch.equal(got["pred"].long(), got["logits"].argmax(1))  # lowest index on ties included
    loss_sum, correct, conf = got["kernel"].infer_stats(got["stats"])
    bound = float(ref["bound_loss"].sum())
    print(f"{case}: loss sum err {abs(loss_sum - float(ref['row_loss'].sum())):.3e}, bound {bound:.3e}")
    assert abs(loss_sum - float(ref["row_loss"].sum())) <= bound
    want_correct, want_conf = ic.expected_counts(ref, got["pred"], C)
    assert correct == want_correct and torch.equal(conf, want_conf) and int(conf.sum()) == n


@pytest.mark.parametrize("case", ic.LOGITS100)
def test_probabilities_are_finite_at_logits_of_100(case, cuda):
    got = _launch(case, cuda)
    assert float(got["logits"].abs().max()) >= 100.0
    assert bool(torch.isfinite(got["probs"]).all()) and float(got["probs"].min()) >= 0.0
    loss_sum, _, _ = got["kernel"].infer_stats(got["stats"])
    assert loss_sum == loss_sum and abs(loss_sum) != float("inf")


@pytest.mark.parametrize("case", ic.NORM)
def test_norm_in_the_gather_equals_normalised_inputs(case, cuda):
    """The case's bound already holds with norm on (the table test); the zero-std column must come through as
    (x - mean) / 1, and turning norm off must change the answer."""
    d = ic.inputs(case)
    assert int((d["raw_std"] == 0).sum()) == 1
    on = _launch(case, cuda)
    off = _launch(case, cuda, norm=None)
    assert not torch.equal(on["logits"], off["logits"])
    ref = ic.reference(case)
    assert bool(((on["logits"].double() - ref["logits"]).abs() <= ref["bound_z"]).all())


def test_without_labels_no_statistics_are_written(cuda):
    case = "5x128x128x2-n165-g2"
    got = _launch(case, cuda, with_y=False)
    assert bool((got["stats"] == -1).all())
    ref = ic.reference(case)
    assert bool(((got["logits"].double() - ref["logits"]).abs() <= ref["bound_z"]).all())


@pytest.mark.parametrize("missing", ["logits", "probs", "pred", "all"])
def test_every_optional_output_null_in_turn(missing, cuda):
    case = "7x48x32x3-n165-g2"
    full = _launch(case, cuda)
    outs = () if missing == "all" else tuple(o for o in ("logits", "probs", "pred") if o != missing)
    got = _launch(case, cuda, outs=outs)
    for o in ("logits", "probs", "pred"):
        if o in outs:
            assert torch.equal(got[o], full[o])
        else:  # untouched
            assert bool((got[o] == (-7 if o == "pred" else POISON)).all())
    assert torch.equal(got["stats"], full["stats"])


@pytest.mark.parametrize("case", ["5x128x128x2-n165-g2", "5x64x2-n165-norm", "32x128x128x4-n33"])
def test_statistics_are_bit_identical_across_grids_and_runs(case, cuda):
    runs = [_launch(case, cuda, grid=g)["stats"].cpu() for g in (1, 3, None, None)]
    for r in runs[1:]:
        assert torch.equal(r, runs[0])


def test_statistics_over_many_slots_per_workgroup_and_tiles_per_slot(cuda):
    """5,000 tiles: 2 tiles per slot, 2,500 slots - against a chunked torch fp64 sum of the launch's own logits,
    at grid 7, 1024 and the default (bit-identical)."""
    dims = [5, 64, 2]
    n = 160000 - 9
    g = torch.Generator().manual_seed(5)
    p = ((torch.rand(ic.num_params(dims), generator=g) * 2 - 1) * 0.5).to(cuda)
    X = torch.randn(n, 5, generator=g).to(cuda)
    Y = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).to(cuda)
    kern = FusedMLPKernel(dims, bmax=1024)
    assert native().mlp_infer_ws_bytes(dims, n) == 2500 * 18 * 8
    logits = torch.empty(n, 2, device=cuda)
    outs = []
    for grid in (7, 1024, None):
        stats = torch.zeros(6, dtype=torch.int64, device=cuda)
        kern.infer(p, X, n, Y=Y, logits_out=logits, stats_out=stats, grid=grid)
        outs.append(stats.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    loss_sum, correct, conf = kern.infer_stats(outs[0])
    z = logits.double()
    y = Y.long()
    rows = torch.logsumexp(z, 1) - z.gather(1, y[:, None])[:, 0]
    # per row: the fp32 evaluation of mx + log(sum) - z_y from the launch's own logits (infer_cases' CE bound without
    # the logit term)
    bound = float((16 * ic.U + 4 * ic.U * (z.max(1).values.abs() + z.gather(1, y[:, None])[:, 0].abs() + 2)).sum())
    assert abs(loss_sum - float(rows.sum())) <= bound
    pred = z.argmax(1)
    assert correct == int((pred == y).sum()) and torch.equal(conf, ic.confusion(y, pred, 2).cpu())


@pytest.mark.parametrize("dims", [[5, 128, 128, 2], [5, 64, 2]])
def test_launcher_refuses_a_parameter_pointer_off_the_16_byte_boundary(dims, cuda):
    """The host check the launcher shares with the batch-tiled trainer (csrc/mlp_tile_fwd.h): W1 is read as float4.
    One float into an aligned allocation is refused with nothing written; the aligned view goes through."""
    nat, n, C, P = native(), 33, dims[-1], ic.num_params(dims)
    g = torch.Generator().manual_seed(7)
    buf = torch.zeros(P + 1, device=cuda)
    assert buf.data_ptr() % 16 == 0
    X = torch.randn(n, dims[0], generator=g).to(cuda)
    Y = torch.randint(0, C, (n,), generator=g, dtype=torch.int32).to(cuda)
    ws = torch.full((nat.mlp_infer_ws_bytes(dims, n) // 8,), -1, dtype=torch.int64, device=cuda)
    stats = torch.full((2 + C * C,), -1, dtype=torch.int64, device=cuda)
    logits, probs = torch.full((n, C), POISON, device=cuda), torch.full((n, C), POISON, device=cuda)
    pred = torch.full((n,), -7, dtype=torch.int32, device=cuda)

    def run(p):
        p.copy_((torch.rand(P, generator=g) * 2 - 1) * 0.5)
        nat.mlp_infer(dims, ptr(p), ptr(X), X.stride(0), 0, ptr(Y), n, 0, 0, 0, ptr(logits), ptr(probs), ptr(pred),
                      ptr(ws), ws.numel() * 8, ptr(stats), 0, stream_handle())
        torch.cuda.synchronize()

    with pytest.raises(RuntimeError, match="invalid"):
        run(buf[1:P + 1])
    torch.cuda.synchronize()
    assert bool((logits == POISON).all()) and bool((probs == POISON).all()) and bool((pred == -7).all())
    assert bool((ws == -1).all()) and bool((stats == -1).all())
    run(buf[:P])
    assert bool(torch.isfinite(logits).all()) and bool((logits != POISON).all())
    assert torch.equal(pred.long(), logits.argmax(1)) and int(stats[2:].sum()) == n


def test_launcher_refuses_an_unsupported_shape_and_a_short_workspace(cuda):
    nat = native()
    p = torch.zeros(4096, device=cuda)
    X = torch.zeros(64, 40, device=cuda)
    Y = torch.zeros(64, dtype=torch.int32, device=cuda)
    ws = torch.zeros(64, dtype=torch.int64, device=cuda)
    stats = torch.zeros(18, dtype=torch.int64, device=cuda)

    def run(dims, n, ws_bytes):
        nat.mlp_infer(dims, ptr(p), ptr(X), X.stride(0), 0, ptr(Y), n, 0, 0, 0, 0, 0, 0, ptr(ws), ws_bytes, ptr(stats),
                      0, stream_handle())

    for dims in ([33, 64, 2], [5, 24, 2], [5, 64, 5], [5, 64, 64, 64, 2]):
        assert not FusedMLPKernel.infer_supported(dims) and nat.mlp_infer_ws_bytes(dims, 64) == 0
        with pytest.raises(RuntimeError, match="invalid"):
            run(dims, 64, 64 * 8)
    need = nat.mlp_infer_ws_bytes([5, 64, 2], 64)
    assert need == 2 * 18 * 8
    with pytest.raises(RuntimeError, match="invalid"):
        run([5, 64, 2], 64, need - 8)
    with pytest.raises(RuntimeError, match="invalid"):
        run([5, 64, 2], 0, need)
    run([5, 64, 2], 64, need)  # the same call with enough workspace goes through
    torch.cuda.synchronize()
    assert int(stats[2:6].sum()) == 64
    with pytest.raises(ValueError):
        FusedMLPKernel([33, 64, 2], bmax=4).infer(p[: ic.num_params([33, 64, 2])], X, 8)

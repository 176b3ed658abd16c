"""The fused linear head on stored rows (include/sgl_linear_rows.h; device.linear_class_loss_rows, device.linear_wgrad_rows,
linear_cross_entropy(rows=...), fused_head="in_place") on a real MI355X: run with `-m gpu`.

Two references per case.  (1) float64 numpy on x64 = table[idx] widened exactly, with the tolerances of tests/test_gpu_linear_head.py
(the header's bounds of K21, evaluated on float64 quantities).  (2) The contract: every output bit-equal to the parent path,
linear_class_loss(gather_rows(table, idx), ...) / linear_wgrad(...), under the same loss_blocks."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from sgl_amd import _lib, config
from sgl_amd import device as dev
from sgl_amd.models import base_model
from sgl_amd.models.homo import SGC
from sgl_amd.tricks import classification as cl
from test_gpu_linear_head import U, WEIGHT, cuda, dz_tol, loss_tol, same, softmax_parts, wgrad_tol  # noqa: F401 (cuda: the fixture)

pytestmark = pytest.mark.gpu
DTYPES = (torch.float32, torch.bfloat16)
# table rows, m (None: idx=None, every row), d, C, layout of the table / W / dz, loss_blocks.  m: one live lane, a partial second row
# tile, several batches; d: below one MFMA step, no multiple of 4 (contiguous: a bf16 pitch that is no multiple of 4 elements), the
# column-chunk path (d = 600; d = 130 at C = 172, 256); C: every compiled tile count; the strided grid and a multi-block fold
CASES = ((1, 1, 1, 1, "contiguous", 0), (40, 33, 7, 3, "view", 0), (40, 33, 7, 3, "contiguous", 0), (40, 33, 100, 47, "pitch", 0),
         (2053, 1031, 100, 47, "contiguous", 1), (2053, 1031, 100, 47, "view", 3), (2053, 1031, 130, 33, "pitch", 3),
         (40, 33, 600, 65, "contiguous", 0), (2053, 1031, 7, 172, "pitch", 0), (40, 33, 130, 256, "view", 0),
         (2053, 1031, 600, 100, "contiguous", 3), (1031, None, 130, 172, "pitch", 3))


def in_layout(src, layout):   # contiguous; alloc_rows' pitch in src's dtype (wide lanes); columns 1 .. d of a NaN-filled [n, d + 3] buffer
    if layout == "contiguous":
        return src
    n, d = src.shape
    out = (dev.alloc_rows(n, d, src.device, dtype=src.dtype) if layout == "pitch"
           else torch.full((n, d + 3), float("nan"), dtype=src.dtype, device=src.device)[:, 1:d + 1])
    out.copy_(src)
    return out


def inputs(n_rows, m, d, c, dtype, cuda):
    """host: the index (unsorted, duplicates, negative entries, row 0 and the table's last row), x64 = table[idx] widened exactly;
    device: the table in `dtype`, W, b, mixed live / ignored labels"""
    rng = np.random.default_rng(n_rows * 1000003 + d * 1009 + c)
    table = torch.from_numpy(rng.standard_normal((n_rows, d)).astype(np.float32)).to(dtype)
    w = torch.from_numpy((rng.standard_normal((c, d)) * 2 / np.sqrt(d)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(c).astype(np.float32))
    at = np.arange(n_rows) if m is None else rng.integers(-n_rows, n_rows, m)
    if m is not None:
        at[:3] = (-1, 0, n_rows - 1)[:m]
    y = rng.integers(0, c, len(at))
    y[::5] = -1
    return at, table.double().numpy()[at], table.to(cuda), w.to(cuda), b.to(cuda), torch.from_numpy(y).to(cuda)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("n_rows,m,d,c,layout,blocks", CASES)
def test_rows_against_float64_and_the_gathered_path(cuda, dtype, n_rows, m, d, c, layout, blocks):
    at, x64, table, w, b, y = inputs(n_rows, m, d, c, dtype, cuda)
    n = len(at)
    x, wt = in_layout(table, layout), in_layout(w, layout)
    # the index as a device tensor, as host indices (validated on the host), or None
    idx = None if m is None else (torch.from_numpy(at).to(cuda) if blocks == 0 else at)
    dz_out = in_layout(torch.full((n, c), 7.0, device=cuda), layout)
    try:
        _lib.set_tuning("loss_blocks", blocks)
        dz, loss, pred, z = dev.linear_class_loss_rows(x, idx, wt, b, y, WEIGHT, dz=dz_out, row_loss=True, pred=True, logits=True)
        again = dev.linear_class_loss_rows(x, idx, wt, b, y, WEIGHT, dz=True, row_loss=True, pred=True, logits=True)
        only = dev.linear_class_loss_rows(x, idx, wt, b, None, 1.0, pred=True)[2]
        dw, db = dev.linear_wgrad_rows(x, idx, dz)
        g = dev.gather_rows(x, at)                                       # the parent path: a float32 copy of the batch, then K21
        parent = dev.linear_class_loss(g, wt, b, y, WEIGHT, dz=True, row_loss=True, pred=True, logits=True)
        parent_w = dev.linear_wgrad(g, parent[0])
        tol_w, tol_b = wgrad_tol(n, d, c, np.abs(dz.cpu().numpy().astype(np.float64)), np.abs(x64))
    finally:
        _lib.set_tuning("loss_blocks", 0)
    assert dz is dz_out and all(same(a, p) for a, p in zip(again + (only,), (dz, loss, pred, z, pred))), "two runs differ"
    assert all(same(a, p) for a, p in zip((dz, loss, pred, z, dw, db), parent + parent_w)), "not the bits of the gathered path"
    if layout == "view":                                               # the pads of an output are not written
        assert bool(torch.isnan(dz_out._base[:, 0]).all()) and bool(torch.isnan(dz_out._base[:, c + 1:]).all())
    w64, b64, y64 = w.double().cpu().numpy(), b.double().cpu().numpy(), y.cpu().numpy()
    z64 = x64 @ w64.T + b64
    e = (d + 3) * U * (np.abs(x64) @ np.abs(w64).T + np.abs(b64))
    mx, lse, p, loss64, dz64 = softmax_parts(z64, y64, WEIGHT)
    ei, rows = e.max(1), np.arange(n)
    zg, lg, dg, pg = (t.cpu().numpy().astype(np.float64) for t in (z, loss, dz, pred))
    ratios = dict(z=np.abs(zg - z64) / e, loss=np.abs(lg - loss64) / loss_tol(ei, c, lse, loss64),
                  dz=np.abs(dg - dz64) / dz_tol(ei, c, z64, mx, p, WEIGHT),
                  dw=np.abs(dw.cpu().numpy() - dg.T @ x64) / np.maximum(tol_w, 1e-300),
                  db=np.abs(db.cpu().numpy() - dg.sum(0)) / np.maximum(tol_b, 1e-300))
    print((n_rows, m, d, c, layout, blocks), {k: float(v.max()) for k, v in ratios.items()})
    for name, ratio in ratios.items():
        assert np.isfinite(ratio).all() and ratio.max() <= 1.0, (name, float(ratio.max()))
    pi = pg.astype(np.int64)
    assert not lg[y64 < 0].any() and not dg[y64 < 0].any(), "a row that is not live has a loss or a gradient"
    assert pi.min() >= 0 and pi.max() < c and (z64[rows, pi] >= mx - 2 * ei).all(), "pred is not within 2 E of the row's maximum"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_an_index_out_of_range_reads_as_nan_and_does_not_trap(cuda, dtype):
    at, _, table, w, b, y = inputs(40, 33, 100, 47, dtype, cuda)
    bad = at.copy()
    bad[5], bad[9] = 40, -41                                           # one past either end; the parent path gets a valid stand-in
    dz, loss, pred, z = dev.linear_class_loss_rows(table, torch.from_numpy(bad).to(cuda), w, b, y, WEIGHT, dz=True, row_loss=True,
                                                   pred=True, logits=True)
    torch.cuda.synchronize()                                           # the call returns normally
    want = dev.linear_class_loss(dev.gather_rows(table, at), w, b, y, WEIGHT, dz=True, row_loss=True, pred=True, logits=True)
    keep = torch.ones(33, dtype=torch.bool, device=cuda)
    keep[[5, 9]] = False
    assert bool(torch.isnan(z[~keep]).all()) and bool((pred[~keep] == 0).all())
    assert all(same(a[keep], p[keep]) for a, p in zip((dz, loss, pred, z), want))


def test_mismatched_shapes_are_refused(cuda):
    x, y = torch.zeros((8, 16), device=cuda).bfloat16(), torch.zeros(3, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="row length"):
        dev.linear_class_loss_rows(x, [0, 1], torch.zeros((3, 15), device=cuda), None, None, 1.0, pred=True)
    with pytest.raises(ValueError, match="labels"):                     # labels go with the index, not with the table
        dev.linear_class_loss_rows(x, [0, 1], torch.zeros((3, 16), device=cuda), None, y, 1.0, row_loss=True)
    with pytest.raises(ValueError, match="same number of rows"):
        dev.linear_wgrad_rows(x, [0, 1], torch.zeros((8, 3), device=cuda))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("reduction,check", (("mean", True), ("sum", True), ("mean", False)))
def test_linear_cross_entropy_rows_against_torch_float64(cuda, dtype, reduction, check):
    n_rows, n, d, c = 2053, 1031, 100, 47
    at, x64, table, w0, b0, y0 = inputs(n_rows, n, d, c, dtype, cuda)
    yk = y0.cpu().numpy()
    y = torch.from_numpy(np.where(yk < 0, -100, yk))
    ref = [torch.from_numpy(x64), w0.double().cpu().requires_grad_(), b0.double().cpu().requires_grad_()]
    want = F.cross_entropy(F.linear(*ref), y, reduction=reduction)
    want.backward()
    w64, b64, want = ref[1].detach().numpy(), ref[2].detach().numpy(), float(want.detach())
    got = []
    for rows in (at, None):                                            # in place, then the parent path on the gathered copy
        w, b = w0.clone().requires_grad_(), b0.clone().requires_grad_()
        x = table if rows is not None else dev.gather_rows(table, at)
        loss, pred = cl.linear_cross_entropy(x, w, b, y.to(cuda), reduction=reduction, check=check, return_pred=True, rows=rows)
        loss.backward()
        got.append((loss.detach(), pred, w.grad, b.grad))
    assert all(same(a, p) for a, p in zip(*got)), "not the bits of linear_cross_entropy on the gathered rows"
    loss, _, w_grad, b_grad = got[0]
    z64 = x64 @ w64.T + b64
    live, ei = yk >= 0, ((d + 3) * U * (np.abs(x64) @ np.abs(w64).T + np.abs(b64))).max(1)
    m, lse, p, loss64, dz1 = softmax_parts(z64, yk, 1.0)
    scale = 1.0 / live.sum() if reduction == "mean" else 1.0
    tol = scale * loss_tol(ei, c, lse, loss64)[live].sum() + 2.0 ** -23 * abs(want)
    assert abs(float(loss) - want) <= tol, (float(loss), want, tol)
    # the weight of dz is rounded to float32 (and applied in two factors with check=False): 3 roundings on top of the header's bound
    dz64 = dz1 * scale
    tol_dz = dz_tol(ei, c, z64, m, p, scale) * live[:, None] + 3 * 2.0 ** -23 * np.abs(dz64)
    tol_w, tol_b = wgrad_tol(n, d, c, np.abs(dz64) + tol_dz, np.abs(x64))
    tol_w, tol_b = tol_w + tol_dz.T @ np.abs(x64), tol_b + tol_dz.sum(0)
    for name, grad, ref_grad, t in (("weight", w_grad, ref[1].grad, tol_w), ("bias", b_grad, ref[2].grad, tol_b)):
        ratio = np.abs(grad.cpu().numpy().astype(np.float64) - ref_grad.numpy()) / t
        assert ratio.max() <= 1.0, (name, float(ratio.max()))


@pytest.mark.parametrize("hop_dtype", ("float32", "bfloat16"))
def test_three_steps_and_an_evaluation_in_place_against_fused(cuda, monkeypatch, hop_dtype):
    """train on cuda:0, evaluate on "cuda" (no index: the current device), then node_classification with its default device"""
    n, d, c = 300, 20, 5
    rng = np.random.default_rng(3)
    adj = sp.random(n, n, density=0.02, random_state=3, format="csr", dtype=np.float32)
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()
    feats = rng.standard_normal((n, d)).astype(np.float32)
    labels = torch.from_numpy(rng.integers(0, c, n)).to(cuda)
    train_idx, val_idx, test_idx = np.arange(0, n, 2), np.arange(1, n, 4), np.arange(3, n, 4)
    monkeypatch.setattr(config, "hop_dtype", hop_dtype)
    torch.manual_seed(0)
    models = [SGC(2, d, c) for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    got = []
    for model, mode in zip(models, (True, "in_place")):
        model.preprocess(adj, feats)
        model.to(cuda)
        assert model._processed_feature.dtype == dev.hop_torch_dtype(hop_dtype)
        if mode == "in_place":                                         # this mode never gathers: take_rows() without arguments raises
            monkeypatch.setattr(base_model, "take_rows", lambda: None)
        opt = torch.optim.SGD(model.parameters(), lr=0.5)
        steps = [cl.train(model, train_idx, labels, cuda, opt, fused_head=mode) for _ in range(3)]
        accs = cl.evaluate(model, val_idx, test_idx, labels, "cuda", fused_head=mode)
        task = cl.node_classification(model, adj, feats, labels, train_idx, val_idx, test_idx, 2, 0.1, 0.0, fused_head=mode)
        got.append((steps, accs, model._base_model.linear, task))
    assert got[0][:2] == got[1][:2] and got[0][3] == got[1][3], "losses and accuracies differ"
    assert same(got[0][2].weight.detach(), got[1][2].weight.detach()) and same(got[0][2].bias.detach(), got[1][2].bias.detach())

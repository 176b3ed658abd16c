"""The linear head fused with its loss (csrc/sgl_linear_head.hip, include/sgl_linear_head.h; device.linear_class_loss, device.linear_wgrad,
tricks.classification.linear_cross_entropy, fused_head=True) on a real MI355X: run with `-m gpu`.

The reference is float64 numpy / torch on the host.  Every tolerance is the header's bound evaluated on float64 quantities (u = 2^-24):
logits E = (d + 3) u (sum |w x| + |b|); row_loss 2 E_i + (C + 16) 2^-23 + 2^-23 (|lse| + |L|); dz |w| (p (expm1(2 E_i) + (C + 8 + |Z - m|)
2^-23) + 2^-23); pred Z[i, pred] >= max - 2 E_i on EVERY row; dW, db (R / 2 + B + 8) u sum |dz x| with R, B from sgl_linear_wgrad_rule."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.models.homo import GAMLP, SGC
from sgl_amd.tricks import classification as cl

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
LAYOUTS = ("contiguous", "pitch", "view")
# n, d, C, layout, loss_blocks, labels: every compiled tile count (C), a partial row tile / two tiles / several batches (n), below one
# MFMA step, not a multiple of 8 and the column-chunk path (d = 600; d = 130 at C = 172, 256), the strided grid and a multi-block fold
CASES = ((1, 1, 1, "contiguous", 0, "mixed"), (33, 7, 3, "view", 0, "mixed"), (33, 100, 47, "pitch", 0, "mixed"),
         (1031, 100, 47, "contiguous", 1, "mixed"), (1031, 100, 47, "view", 3, "mixed"), (1031, 130, 33, "pitch", 3, "mixed"),
         (33, 600, 65, "contiguous", 0, "mixed"), (1031, 7, 172, "pitch", 0, "mixed"), (33, 130, 256, "view", 0, "ignored"),
         (1031, 600, 256, "contiguous", 3, "mixed"), (33, 1, 65, "pitch", 0, "mixed"))
WEIGHT = 0.37
_REF = {}


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def same(a, b):
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t    # noqa: E731
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def in_layout(host, layout, device):
    """contiguous; the padded pitch of alloc_rows (16-byte lanes); columns 1 .. d of a NaN-filled [n, d + 3] buffer (4-byte lanes)"""
    src = torch.from_numpy(np.ascontiguousarray(host)).to(device)
    if layout == "contiguous":
        return src
    n, d = host.shape
    out = dev.alloc_rows(n, d, device) if layout == "pitch" else torch.full((n, d + 3), float("nan"), device=device)[:, 1:d + 1]
    out.copy_(src)
    return out


def softmax_parts(z, y, w):
    """float64: (row max m, lse, softmax p, row losses, dZ) for labels y (-1: not live) and weight w"""
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    p = np.exp(z - lse[:, None])
    live, rows = y >= 0, np.arange(len(y))
    onehot = np.zeros_like(z)
    onehot[rows[live], y[live]] = 1.0
    return m, lse, p, np.where(live, lse - z[rows, np.maximum(y, 0)], 0.0), w * (p - onehot) * live[:, None]


def reference(n, d, c, labels):
    """the inputs in float32 and everything float64 the assertions need -- once per case, left unchanged"""
    key = (n, d, c, labels)
    if key not in _REF:
        rng = np.random.default_rng(n * 1000003 + d * 1009 + c)
        x = rng.standard_normal((n, d)).astype(np.float32)
        w = (rng.standard_normal((c, d)) * 2 / np.sqrt(d)).astype(np.float32)
        b = rng.standard_normal(c).astype(np.float32)
        y = rng.integers(0, c, n)
        y[::5] = -1                                                    # ignored rows (row 0 too: n = 1 has none live)
        if labels == "ignored":
            y[:] = -1
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        z = x64 @ w64.T + b
        e = (d + 3) * U * (np.abs(x64) @ np.abs(w64).T + np.abs(b))
        _REF[key] = dict(x=x, w=w, b=b, y=y, z=z, e=e, parts=softmax_parts(z, y, WEIGHT))
    return _REF[key]


def loss_tol(ei, c, lse, loss):
    return 2 * ei + (c + 16) * 2.0 ** -23 + 2.0 ** -23 * (np.abs(lse) + np.abs(loss))


def dz_tol(ei, c, z, m, p, w):
    return abs(w) * (p * (np.expm1(2 * ei)[:, None] + (c + 8 + np.abs(z - m[:, None])) * 2.0 ** -23) + 2.0 ** -23)


def wgrad_tol(n, d, c, absdz, absx):
    """(tolerance of dW [C, d], of db [C]) under the current loss_blocks"""
    rule = (ctypes.c_int64 * 5)()
    _lib.check(_lib.lib().sgl_linear_wgrad_rule(n, d, c, rule), "sgl_linear_wgrad_rule")
    depth = (rule[1] / 2 + rule[0] + 8) * U
    return depth * (absdz.T @ absx), depth * absdz.sum(0)


@pytest.mark.parametrize("n,d,c,layout,blocks,labels", CASES)
def test_every_output_against_float64(cuda, n, d, c, layout, blocks, labels):
    r = reference(n, d, c, labels)
    m, lse, p, loss64, dz64 = r["parts"]
    ei, rows = r["e"].max(1), np.arange(n)
    x, w = in_layout(r["x"], layout, cuda), in_layout(r["w"], layout, cuda)
    b, y = torch.from_numpy(r["b"]).to(cuda), torch.from_numpy(r["y"]).to(cuda)
    dz_out = in_layout(np.full((n, c), 7.0, np.float32), layout, cuda)
    try:
        _lib.set_tuning("loss_blocks", blocks)
        dz, loss, pred, z = dev.linear_class_loss(x, w, b, y, WEIGHT, dz=dz_out, row_loss=True, pred=True, logits=True)
        again = dev.linear_class_loss(x, w, b, y, WEIGHT, dz=True, row_loss=True, pred=True, logits=True)
        only = dev.linear_class_loss(x, w, b, None, 1.0, pred=True)[2]         # the arg-max-only launch: no labels, no exp
        dw, db = dev.linear_wgrad(x, dz)
        dw2, db2 = dev.linear_wgrad(x, dz)
        tol_w, tol_b = wgrad_tol(n, d, c, np.abs(dz.cpu().numpy().astype(np.float64)), np.abs(r["x"].astype(np.float64)))
    finally:
        _lib.set_tuning("loss_blocks", 0)
    assert dz is dz_out and all(same(a, g) for a, g in zip(again, (dz, loss, pred, z))) and same(only, pred), "two runs differ"
    assert same(dw, dw2) and same(db, db2), "two weight gradients differ"
    if layout == "view":                                               # the pads of an output are not written
        assert bool(torch.isnan(dz_out._base[:, 0]).all()) and bool(torch.isnan(dz_out._base[:, c + 1:]).all())
    zg, lg, dg, pg = z.cpu().numpy().astype(np.float64), loss.cpu().numpy().astype(np.float64), dz.cpu().numpy().astype(np.float64), pred.cpu().numpy()
    ratios = dict(z=np.abs(zg - r["z"]) / r["e"], loss=np.abs(lg - loss64) / loss_tol(ei, c, lse, loss64),
                  dz=np.abs(dg - dz64) / dz_tol(ei, c, r["z"], m, p, WEIGHT),
                  dw=np.abs(dw.cpu().numpy() - dg.T @ r["x"].astype(np.float64)) / np.maximum(tol_w, 1e-300),
                  db=np.abs(db.cpu().numpy() - dg.sum(0)) / np.maximum(tol_b, 1e-300))
    print((n, d, c, layout, blocks), {k: float(v.max()) for k, v in ratios.items()})
    for name, ratio in ratios.items():
        assert np.isfinite(ratio).all() and ratio.max() <= 1.0, (name, float(ratio.max()))
    dead = r["y"] < 0
    assert not lg[dead].any() and not dg[dead].any(), "a row that is not live has a loss or a gradient"
    assert pg.min() >= 0 and pg.max() < c and (r["z"][rows, pg] >= m - 2 * ei).all(), "pred is not within 2 E of the row's maximum"


@pytest.mark.parametrize("n,d,c", ((1031, 100, 47), (33, 130, 172)))
def test_the_bits_do_not_depend_on_the_layout(cuda, n, d, c):
    r = reference(n, d, c, "mixed")
    b, y = torch.from_numpy(r["b"]).to(cuda), torch.from_numpy(r["y"]).to(cuda)
    got = []
    for layout in LAYOUTS:
        x, w = in_layout(r["x"], layout, cuda), in_layout(r["w"], layout, cuda)
        outs = dev.linear_class_loss(x, w, b, y, WEIGHT, dz=in_layout(np.zeros((n, c), np.float32), layout, cuda), row_loss=True, pred=True, logits=True)
        got.append(outs + dev.linear_wgrad(x, outs[0]))
    assert all(same(a, g) for other in got[1:] for a, g in zip(other, got[0]))


def test_ties_and_nan_follow_the_class_loss_kernel(cuda):
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.random((33, 9), dtype=np.float32) + 0.5).to(cuda)
    w = torch.from_numpy((rng.standard_normal((7, 9)) * 0.01).astype(np.float32)).to(cuda)
    b = torch.zeros(7, device=cuda)
    w[2] = w[5] = 1.0                                                  # two identical rows with equal bias hold the maximum
    assert bool((dev.linear_class_loss(x, w, b, None, 1.0, pred=True)[2] == 2).all()), "the lower index must win a tie"
    w[4, 1], x[3, 0] = float("nan"), float("nan")                       # logit 4 of every row is NaN; every logit of row 3
    y = torch.zeros(33, dtype=torch.int64, device=cuda)
    dz, loss, pred, z = dev.linear_class_loss(x, w, b, y, 1.0, dz=True, row_loss=True, pred=True, logits=True)
    want = dev.class_loss_grad(z, y, 1.0, dz=True, row_loss=True, pred=True)
    expect = torch.full((33,), 4, device=cuda)
    expect[3] = 0
    assert torch.equal(pred, expect) and torch.equal(pred, want[2]), "a NaN counts as the maximum, the first NaN wins"
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dz).all()) and bool(torch.isnan(want[1]).all())


@pytest.mark.parametrize("reduction,check", (("mean", True), ("sum", True), ("mean", False)))
def test_linear_cross_entropy_against_torch_float64(cuda, reduction, check):
    n, d, c = 1031, 100, 47
    r = reference(n, d, c, "mixed")
    y = np.where(r["y"] < 0, -100, r["y"])
    ref = [torch.from_numpy(r[k].astype(np.float64)).requires_grad_(k != "x") for k in ("x", "w", "b")]
    want = F.cross_entropy(F.linear(*ref), torch.from_numpy(y), reduction=reduction)
    want.backward()
    x, w, b = (torch.from_numpy(r[k]).to(cuda).requires_grad_(k != "x") for k in ("x", "w", "b"))
    loss, pred = cl.linear_cross_entropy(x, w, b, torch.from_numpy(y).to(cuda), reduction=reduction, check=check, return_pred=True)
    loss.backward()
    assert x.grad is None and loss.dtype == torch.float32 and pred.dtype == torch.int64
    m, lse, p, loss64, _ = r["parts"]
    scale = 1.0 / (r["y"] >= 0).sum() if reduction == "mean" else 1.0
    ei, live = r["e"].max(1), r["y"] >= 0
    tol = scale * loss_tol(ei, c, lse, loss64)[live].sum() + 2.0 ** -23 * abs(float(want.detach()))
    assert abs(float(loss.detach()) - float(want.detach())) <= tol, (float(loss.detach()), float(want.detach()), tol)
    # the weight of dz is rounded to float32 (and applied in two factors with check=False): 3 roundings on top of the header's bound
    dz64 = r["parts"][4] / WEIGHT * scale
    tol_dz = dz_tol(ei, c, r["z"], m, p, scale) * live[:, None] + 3 * 2.0 ** -23 * np.abs(dz64)
    absx = np.abs(r["x"].astype(np.float64))
    tol_w, tol_b = wgrad_tol(n, d, c, np.abs(dz64) + tol_dz, absx)
    tol_w, tol_b = tol_w + tol_dz.T @ absx, tol_b + tol_dz.sum(0)
    for name, got, ref_grad, t in (("weight", w.grad, ref[1].grad, tol_w), ("bias", b.grad, ref[2].grad, tol_b)):
        ratio = np.abs(got.cpu().numpy().astype(np.float64) - ref_grad.numpy()) / t
        print(reduction, check, name, float(ratio.max()))
        assert ratio.max() <= 1.0, (name, float(ratio.max()))


def test_refusals(cuda):
    x, y = torch.zeros((8, 16), device=cuda), torch.zeros(8, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="256"):
        dev.linear_class_loss(x, torch.zeros((257, 16), device=cuda), None, y, 1.0, row_loss=True)
    with pytest.raises(ValueError, match="256"):
        cl.linear_cross_entropy(x, torch.zeros((257, 16), device=cuda), None, y)
    with pytest.raises(ValueError, match="bfloat16"):
        dev.linear_class_loss(x.bfloat16(), torch.zeros((3, 16), device=cuda), None, y, 1.0, row_loss=True)
    with pytest.raises(ValueError, match="bfloat16"):
        dev.linear_wgrad(x.bfloat16(), torch.zeros((8, 3), device=cuda))
    model = GAMLP(2, 16, 3, 8, 2).to(cuda)
    with pytest.raises(ValueError, match="LogisticRegression"):
        cl.train(model, range(8), y, cuda, torch.optim.SGD(model.parameters(), lr=0.1), fused_head=True)
    with pytest.raises(ValueError, match="callable"):
        cl.train(SGC(2, 16, 3), range(8), y, cuda, None, loss_fn=F.cross_entropy, fused_head=True)


def test_three_training_steps_fused_against_unfused(cuda):
    """SGC on a 300-node graph, plain SGD.  Both routes are float32 evaluations of the same float64 gradient descent; `dev` bounds
    how far one can be from it after each step: dev + lr (the bound of the computed gradient at the float64 iterate + the change of the
    exact gradient over dev: dZ moves by at most p expm1(2 delta), delta = max_i |x_i|_1 dev_W + dev_b) + the rounding of the update.
    The fused route is held to dev against float64, the two routes to 2 dev against each other."""
    n, d, c, lr, steps = 300, 20, 5, 0.5, 3
    rng = np.random.default_rng(3)
    adj = sp.random(n, n, density=0.02, random_state=3, format="csr", dtype=np.float32)
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()
    feats = rng.standard_normal((n, d)).astype(np.float32)
    labels = torch.from_numpy(rng.integers(0, c, n)).to(cuda)
    train_idx = np.arange(0, n, 2)
    torch.manual_seed(0)
    models = [SGC(2, d, c) for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    w, b = (models[0].state_dict()[f"_base_model._LogisticRegression__fc.{k}"].double().numpy().copy() for k in ("weight", "bias"))
    history = []
    for model, fused in zip(models, (True, False)):
        model.preprocess(adj, feats)
        model.to(cuda)
        opt = torch.optim.SGD(model.parameters(), lr=lr)
        history.append([cl.train(model, train_idx, labels, cuda, opt, fused_head=fused)[0] for _ in range(steps)])
    x = models[0]._processed_feature[torch.from_numpy(train_idx).to(cuda)].cpu().numpy().astype(np.float64)
    y, m_rows = labels.cpu().numpy()[train_idx], len(train_idx)
    absx, dev_w, dev_b = np.abs(x), 0.0, 0.0
    for step in range(steps):
        z = x @ w.T + b
        ei = ((d + 3) * U * (absx @ np.abs(w).T + np.abs(b))).max(1)
        m, lse, p, loss64, dz = softmax_parts(z, y, 1.0 / m_rows)
        delta = absx.sum(1).max() * dev_w + dev_b
        tol_loss = loss_tol(ei, c, lse, loss64).mean() + 2 * delta + 2.0 ** -23 * loss64.mean()
        for got in (history[0][step], history[1][step]):
            assert abs(got - loss64.mean()) <= tol_loss, (step, got, float(loss64.mean()), tol_loss)
        tol_dz = dz_tol(ei, c, z, m, p, 1.0 / m_rows) + 3 * 2.0 ** -23 * np.abs(dz) + p * np.expm1(2 * delta) / m_rows
        tol_w, tol_b = wgrad_tol(m_rows, d, c, np.abs(dz) + tol_dz, absx)
        gw, gb = dz.T @ x, dz.sum(0)
        dev_w += lr * (tol_w + tol_dz.T @ absx).max() + 2.0 ** -23 * (np.abs(w).max() + lr * np.abs(gw).max() + dev_w)
        dev_b += lr * (tol_b + tol_dz.sum(0)).max() + 2.0 ** -23 * (np.abs(b).max() + lr * np.abs(gb).max() + dev_b)
        w, b = w - lr * gw, b - lr * gb
    fw, fb = (t.detach().cpu().double().numpy() for t in (models[0]._base_model.linear.weight, models[0]._base_model.linear.bias))
    uw, ub = (t.detach().cpu().double().numpy() for t in (models[1]._base_model.linear.weight, models[1]._base_model.linear.bias))
    print("deviation bounds", dev_w, dev_b, "fused off float64", np.abs(fw - w).max(), np.abs(fb - b).max(), "off unfused", np.abs(fw - uw).max())
    assert np.abs(fw - w).max() <= dev_w and np.abs(fb - b).max() <= dev_b
    assert np.abs(fw - uw).max() <= 2 * dev_w and np.abs(fb - ub).max() <= 2 * dev_b

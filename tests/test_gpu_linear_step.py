"""K23, the one-pass training step of the linear head (include/sgl_linear_step.h) on the GPU: row_loss and pred bit-equal to the class
kernel, dW and db against float64 inside the header's bound, the rows entry points bit-equal to the dense one, the autograd route and
three SGD steps of SGC under both new fused_head values."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.models.homo import SGC
from sgl_amd.tricks import classification as cl

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
WEIGHT = 0.37
# every compiled (class tiles, column tiles) instance at its widest, and below one MFMA step; (255, 32) and (31, 256) are outside the rule
SHAPES = ((1, 1), (7, 3), (100, 47), (127, 64), (222, 32), (63, 128))
ROWS = (0, 1, 31, 33, 129, 1031)     # nothing; the tile edge; one tile beyond four wavefronts; several tiles per wavefront
# n, (d, C), layout, loss_blocks: a pitched and a 4-byte-misaligned x, one block and three
LAYOUT_CASES = ((1031, (100, 47), "pitch", 1), (1031, (100, 47), "view", 3), (129, (222, 32), "view", 0), (1031, (63, 128), "pitch", 3))


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def same(a, b):
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t    # noqa: E731
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def in_layout(host, layout, device):
    """contiguous; alloc_rows' padded pitch (16-byte lanes); columns 1 .. d of a NaN-filled buffer (4-byte misaligned lanes)"""
    src = torch.from_numpy(np.ascontiguousarray(host)).to(device)
    if layout == "contiguous":
        return src if len(host) else torch.zeros(host.shape, device=device)   # (numpy's empty array has strides of 0)
    n, d = host.shape
    out = dev.alloc_rows(n, d, device) if layout == "pitch" else torch.full((n, d + 3), float("nan"), device=device)[:, 1:d + 1]
    out.copy_(src)
    return out


def inputs(n, d, c, seed=0):
    rng = np.random.default_rng(n * 1000003 + d * 1009 + c + seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    w = (rng.standard_normal((c, d)) * 2 / np.sqrt(d)).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    y = rng.integers(0, c, n)
    y[::5] = -1                                                        # ignored rows
    y[n // 2:n // 2 + 1] = c                                           # one label out of range: not live either
    return x, w, b, y


def step_bound(x, w, b, y, weight):
    """float64 dW, db and the header's bound of each for the current loss_blocks"""
    n, d = x.shape
    c = w.shape[0]
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    z = x64 @ w64.T + b
    ei = ((d + 3) * U * (np.abs(x64) @ np.abs(w64).T + np.abs(b))).max(1)
    m = z.max(1)
    p = np.exp(z - (m + np.log(np.exp(z - m[:, None]).sum(1)))[:, None])
    live = (y >= 0) & (y < c)
    onehot = np.zeros_like(z)
    onehot[np.arange(n)[live], y[live]] = 1.0
    dz = weight * (p - onehot) * live[:, None]
    tol_dz = abs(weight) * (p * (np.expm1(2 * ei)[:, None] + (c + 8 + np.abs(z - m[:, None])) * 2.0 ** -23) + 2.0 ** -23) * live[:, None]
    blocks, rows = dev.linear_step_rule(n, d, c)[:2]
    depth = (32 * -(-(-(-rows // 32)) // 4) + blocks + 8) * U
    x1 = np.hstack((x64, np.ones((n, 1))))                             # db is column d
    return dz.T @ x1, tol_dz.T @ np.abs(x1) + depth * (np.abs(dz).T @ np.abs(x1))


@pytest.mark.parametrize("n,shape,layout,blocks", [(n, s, "contiguous", 0) for n in ROWS for s in SHAPES] + list(LAYOUT_CASES))
def test_the_step_against_the_class_kernel_and_float64(cuda, n, shape, layout, blocks):
    d, c = shape
    x, w, b, y = inputs(n, d, c)
    xd, wd = in_layout(x, layout, cuda), in_layout(w, layout, cuda)
    bd, yd = torch.from_numpy(b).to(cuda), torch.from_numpy(y).to(cuda)
    try:
        _lib.set_tuning("loss_blocks", blocks)
        got = dev.linear_step(xd, wd, bd, yd, WEIGHT, row_loss=True, pred=True)
        again = dev.linear_step(xd, wd, bd, yd, WEIGHT, row_loss=True, pred=True)
        want, tol = step_bound(x, w, b, y, WEIGHT)
    finally:
        _lib.set_tuning("loss_blocks", 0)
    if n == 0:                                                         # zeros from the fold alone; the rows entry point too
        empty = dev.linear_step_rows(torch.zeros((3, d), device=cuda), torch.zeros(0, dtype=torch.int64, device=cuda), wd, bd, yd, WEIGHT)
        assert not got[0].any() and not got[1].any() and same(empty[0], got[0]) and same(empty[1], got[1]) and got[2].numel() == 0
        return
    _, loss, pred, _ = dev.linear_class_loss(xd, wd, bd, yd, WEIGHT, row_loss=True, pred=True)
    assert same(got[2], loss) and same(got[3], pred), "row_loss / pred are not the class kernel's bits"
    assert all(same(a, g) for a, g in zip(again, got)), "two runs differ"
    have = np.hstack((got[0].cpu().numpy(), got[1].cpu().numpy()[:, None])).astype(np.float64)
    ratio = np.abs(have - want) / np.maximum(tol, 1e-300)
    print((n, d, c, layout, blocks), "dW", float(ratio[:, :d].max(initial=0)), "db", float(ratio[:, d].max()))
    assert np.isfinite(have).all() and ratio.max() <= 1.0, float(ratio.max())


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("shape", ((100, 47), (222, 32), (63, 128)))
def test_the_rows_entry_points_are_the_dense_one_on_the_gathered_rows(cuda, dtype, shape):
    d, c = shape
    x, w, b, _ = inputs(300, d, c)
    table = in_layout(x, "pitch", cuda).to(dtype) if dtype == torch.float32 else torch.from_numpy(x).to(cuda).to(dtype)
    rng = np.random.default_rng(5)
    idx = torch.from_numpy(np.concatenate((rng.permutation(300)[:100], [7, 7, -1, -300, 299], rng.integers(-300, 300, 24)))).to(cuda)
    y = torch.from_numpy(rng.integers(-1, c, idx.numel())).to(cuda)
    wd, bd = torch.from_numpy(w).to(cuda), torch.from_numpy(b).to(cuda)
    got = dev.linear_step_rows(table, idx, wd, bd, y, WEIGHT, row_loss=True, pred=True)
    want = dev.linear_step(dev.gather_rows(table, idx), wd, bd, y, WEIGHT, row_loss=True, pred=True)
    assert all(same(a, g) for a, g in zip(got, want))
    whole = dev.linear_step_rows(table, None, wd, bd, y[:1].expand(300).contiguous(), WEIGHT, pred=True)
    assert all(same(a, g) for a, g in zip(whole, dev.linear_step(table.float(), wd, bd, y[:1].expand(300).contiguous(), WEIGHT, pred=True)))
    idx[3] = 300                                                       # out of range: a row of NaN, no trap
    y[3] = 0
    dw, db, loss, pred = dev.linear_step_rows(table, idx, wd, bd, y, WEIGHT, row_loss=True, pred=True)
    assert bool(torch.isnan(loss[3])) and int(pred[3]) == 0 and bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())
    assert same(loss[4:], got[2][4:]) and same(pred[4:], got[3][4:])


@pytest.mark.parametrize("rows", (False, True))
@pytest.mark.parametrize("reduction,check", (("mean", True), ("sum", True), ("mean", False), ("sum", False)))
def test_linear_cross_entropy_one_pass_against_torch_float64(cuda, reduction, check, rows, n=1031, d=100, c=47):
    x, w, b, y = inputs(n, d, c, seed=1)
    y = np.where((y < 0) | (y >= c), -100, y)
    ref = [torch.from_numpy(t.astype(np.float64)).requires_grad_(k > 0) for k, t in enumerate((x, w, b))]
    want = F.cross_entropy(F.linear(*ref), torch.from_numpy(y), reduction=reduction)
    want.backward()
    xd, wd, bd = (torch.from_numpy(t).to(cuda).requires_grad_(k > 0) for k, t in enumerate((x, w, b)))
    args = dict(reduction=reduction, check=check, return_pred=True, rows=range(n) if rows else None)
    loss, pred = cl.linear_cross_entropy(xd, wd, bd, torch.from_numpy(y).to(cuda), one_pass=True, **args)
    loss.backward()
    plain = cl.linear_cross_entropy(xd, wd.detach(), bd.detach(), torch.from_numpy(y).to(cuda), **args)
    assert same(loss.detach(), plain[0]) and same(pred, plain[1]) and xd.grad is None
    with pytest.raises(RuntimeError, match="twice"):
        loss.backward()
    scale = 1.0 / (y >= 0).sum() if reduction == "mean" else 1.0
    grad64, tol = step_bound(x, w, b, y, scale)
    tol = tol + 3 * 2.0 ** -23 * np.abs(grad64)                        # the weight is rounded to float32, the backward's factor too
    have = np.hstack((wd.grad.cpu().numpy(), bd.grad.cpu().numpy()[:, None])).astype(np.float64)
    assert np.abs(grad64 - np.hstack((ref[1].grad.numpy(), ref[2].grad.numpy()[:, None]))).max() <= 1e-12
    ratio = np.abs(have - grad64) / tol
    print(reduction, check, rows, float(ratio.max()))
    assert ratio.max() <= 1.0, float(ratio.max())


def test_three_training_steps_one_pass_against_fused(cuda):
    """SGC on a 300-node graph, plain SGD, as tests/test_gpu_linear_head.py holds the fused route to float64: after each step the
    weights of a float32 route are within dev of the float64 descent, dev grown by lr (the gradient's bound + the change of the exact
    gradient over dev) + the rounding of the update; two routes are within 2 dev of each other."""
    n, d, c, lr, steps = 300, 20, 5, 0.5, 3
    rng = np.random.default_rng(3)
    adj = sp.random(n, n, density=0.02, random_state=3, format="csr", dtype=np.float32)
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()
    feats = rng.standard_normal((n, d)).astype(np.float32)
    labels = torch.from_numpy(rng.integers(0, c, n)).to(cuda)
    train_idx = np.arange(0, n, 2)
    torch.manual_seed(0)
    models = [SGC(2, d, c) for _ in range(3)]
    for model, mode in zip(models, (True, "one_pass", "one_pass_in_place")):
        model.load_state_dict(models[0].state_dict())
        model.preprocess(adj, feats)
        model.to(cuda)
    w, b = (t.detach().cpu().double().numpy().copy() for t in (models[0]._base_model.linear.weight, models[0]._base_model.linear.bias))
    for model, mode in zip(models, (True, "one_pass", "one_pass_in_place")):
        opt = torch.optim.SGD(model.parameters(), lr=lr)
        for _ in range(steps):
            cl.train(model, train_idx, labels, cuda, opt, fused_head=mode)
        plain = {"one_pass": True, "one_pass_in_place": "in_place"}.get(mode, mode)     # evaluation is that mode's arg-max launch
        assert cl.evaluate(model, train_idx, train_idx, labels, cuda, fused_head=mode) == cl.evaluate(model, train_idx, train_idx, labels, cuda, fused_head=plain)
    x = models[0]._processed_feature[torch.from_numpy(train_idx).to(cuda)].cpu().numpy().astype(np.float64)
    y, absx, dev_w, dev_b = labels.cpu().numpy()[train_idx], np.abs(x), 0.0, 0.0
    for _ in range(steps):
        delta = absx.sum(1).max() * dev_w + dev_b
        grad, tol = step_bound(x.astype(np.float32), w, b, y, 1.0 / len(y))
        p_move = np.expm1(2 * delta) / len(y)                          # dZ moves by at most p expm1(2 delta) <= expm1(2 delta)
        tol = tol + 3 * 2.0 ** -23 * np.abs(grad) + p_move * np.hstack((absx, np.ones((len(y), 1)))).sum(0)[None, :]
        dev_w += lr * tol[:, :d].max() + 2.0 ** -23 * (np.abs(w).max() + lr * np.abs(grad[:, :d]).max() + dev_w)
        dev_b += lr * tol[:, d].max() + 2.0 ** -23 * (np.abs(b).max() + lr * np.abs(grad[:, d]).max() + dev_b)
        w, b = w - lr * grad[:, :d], b - lr * grad[:, d]
    fused = models[0]._base_model.linear.requires_grad_(False)
    for model in models[1:]:
        fc = model._base_model.linear.requires_grad_(False)
        print("bounds", dev_w, dev_b, "off fused", float((fc.weight - fused.weight).abs().max()), float((fc.bias - fused.bias).abs().max()))
        assert np.abs(fc.weight.detach().cpu().double().numpy() - w).max() <= dev_w
        assert float((fc.weight - fused.weight).abs().max()) <= 2 * dev_w and float((fc.bias - fused.bias).abs().max()) <= 2 * dev_b


def test_refusals(cuda):
    x, y = torch.zeros((8, 128), device=cuda), torch.zeros(8, dtype=torch.int64, device=cuda)
    w = torch.zeros((64, 128), device=cuda, requires_grad=True)
    with pytest.raises(ValueError, match="sgl_linear_step_rule"):
        dev.linear_step(x, w.detach(), None, y, 1.0)
    with pytest.raises(ValueError, match="sgl_linear_step_rule"):
        cl.linear_cross_entropy(x, w, None, y, one_pass=True)
    for d, c in ((255, 32), (31, 256)):                                # the two shapes whose instances would spill
        with pytest.raises(ValueError, match="sgl_linear_step_rule"):
            dev.linear_step(torch.zeros((8, d), device=cuda), torch.zeros((c, d), device=cuda), None, y, 1.0)
    wide = SGC(2, 500, 3)
    wide._processed_feature = torch.zeros((8, 500), device=cuda)
    with pytest.raises(ValueError, match="sgl_linear_step_rule"):      # before any step
        cl.train(wide, range(8), y, cuda, None, fused_head="one_pass")
    with pytest.raises(ValueError, match="one_pass"):
        cl.linear_cross_entropy(x[:, :16].clone().requires_grad_(), w[:, :16], None, y, one_pass=True)
    model = SGC(2, 16, 3)
    model._pre_msg_learnable = True
    with pytest.raises(ValueError, match="not learnable"):
        cl.train(model, range(8), y, cuda, None, fused_head="one_pass")

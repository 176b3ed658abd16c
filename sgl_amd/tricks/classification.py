"""Node classification on the MI355X: the loss, the accuracy, the steps and the loop of the reference's first task.

Reference: NodeClassification (sgl/tasks/node_classification.py:11-112) runs `train` + `evaluate` (or their mini-batch forms) per epoch
and a post-processing step at the end (sgl/tasks/utils.py:12-98):

    loss_train = loss_fn(train_output, labels[train_idx]); acc_train = accuracy(train_output, labels[train_idx]); loss_train.backward()

with loss_fn = nn.CrossEntropyLoss() or LogeCrossEntropy (sgl/tricks/utils.py:7-10).  Through torch that is a log-softmax forward, the
NLL gather, an arg-max, the NLL backward and the log-softmax backward: about eight passes over the [B, C] logits and two [B, C]
temporaries.  Here ONE launch (device.class_loss_grad -> sgl_class_loss_grad_f32, csrc/sgl_class_loss.hip) reads the logits once and
writes the per-row losses, dLogits and the predicted classes; the backward multiplies the buffer the forward launch wrote by the
upstream gradient in place.  An epoch's evaluation needs the arg-max alone: the same entry with one output, no exp.

`fused=False` is the torch composition (F.cross_entropy, output.max(1)[1]); both routes are kept and tested, and FUSED_DEFAULT -- what
`fused=None` means -- is the faster of the two as measured by tools/bench_class_loss.py (CHANGELOG, DESIGN K14)."""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from .. import device as dev

__all__ = ["cross_entropy", "loge_cross_entropy", "predict", "accuracy", "train", "mini_batch_train", "evaluate", "mini_batch_evaluate",
           "node_classification", "NodeClassificationResult", "epoch_batches",
           "hetero_node_classification", "HeteroNodeClassification", "HeteroNodeClassificationResult"]

FUSED_DEFAULT = True
LOGE_EPSILON = 1.0 - math.log(2)


class _CrossEntropy(torch.autograd.Function):
    """(loss, pred) of one launch: loss = the float64 sum of the rows' float32 losses times w -- or times `scale`, a device scalar,
    when the mean's divisor never left the device (w is 1 then) -- as float32.  dZ is written by the same launch with weight w and
    handed out once, multiplied in place by the upstream gradient (and by `scale`)."""

    @staticmethod
    def forward(ctx, output, labels, w, scale, want_pred):
        dz, row_loss, pred = dev.class_loss_grad(output, labels, w, dz=True, row_loss=True, pred=want_pred)
        ctx.dz, ctx.scale = dz, scale
        loss = (row_loss.sum(dtype=torch.float64) * (w if scale is None else scale)).to(torch.float32)
        if want_pred:
            ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        dz, ctx.dz = ctx.dz, None
        if dz is None:
            raise RuntimeError("cross_entropy: backward ran twice; the gradient buffer of the forward launch was handed out the first time")
        if ctx.scale is not None:
            g = (g * ctx.scale).to(torch.float32)
        return dz.mul_(g), None, None, None, None


def _as_index(idx, device):
    """row indices of any kind (range, list, ndarray, tensor) as an int64 tensor on `device`"""
    if isinstance(idx, range):
        idx = np.arange(idx.start, idx.stop, idx.step, dtype=np.int64)
    t = idx if torch.is_tensor(idx) else torch.as_tensor(np.asarray(idx))
    return t.reshape(-1).to(device=device, dtype=torch.int64)


def _class_labels(labels, c, n, device, ignore_index, check):
    """(labels as the kernel takes them, live): int64 [n] on `device` with every label that is `ignore_index` or outside [0, c)
    replaced by -1 ("no label"), and the number of the others -- a Python int after check=True's one host read, which raises IndexError
    for a label outside [0, c) that is not `ignore_index`; a device scalar, nothing read, with check=False"""
    t = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels)
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
        raise TypeError("cross_entropy: labels must be class indices (integers); probability targets are not supported")
    t = t.reshape(-1).to(device=device, dtype=torch.int64).contiguous()
    if t.numel() != n:
        raise ValueError(f"cross_entropy: {t.numel()} labels for {n} rows")
    ignored = t == int(ignore_index)
    live = (t >= 0) & (t < c) & ~ignored
    count = live.sum()
    if check:
        stray = ~live & ~ignored
        has_stray, count = (int(v) for v in torch.stack((stray.sum(), count)).tolist()) if n else (0, 0)
        if has_stray:
            first = int(t[stray][0])
            raise IndexError(f"cross_entropy: target {first} is out of bounds for {c} classes")
    return torch.where(live, t, torch.full_like(t, -1)), count


def cross_entropy(output, labels, reduction="mean", ignore_index=-100, check=True, fused=None, return_pred=False):
    """nn.CrossEntropyLoss for class-index targets -- its value and its gradient -- as a float32 scalar on output's device:

        loss = sum_{i live} (logsumexp(output[i]) - output[i, labels[i]]) / (number of live rows)     ("mean"; "sum": without the divisor)

    A row is live when its label is not `ignore_index`.  output: [n, C] float32 CUDA matrix of logits (read in place: padded buffers,
    column views); labels: n integers (tensor, ndarray or list).  check=True makes ONE host read: a label outside [0, C) other than
    `ignore_index` raises IndexError, and the divisor of the mean comes back with it.  check=False reads nothing from the device:
    labels outside [0, C) count as ignored and the live count stays a device scalar, so the mean needs no synchronisation.  As in
    torch, the mean over no live row is NaN.
    fused (None: FUSED_DEFAULT): ONE launch of sgl_class_loss_grad_f32 writes the per-row losses, the arg-max when return_pred=True
    and, when output requires grad, dLogits; the loss is the float64 sum of the float32 row losses; the backward multiplies the buffer
    by the upstream gradient in place (no launch of ours, nothing allocated), so a second backward raises.  fused=False: the torch
    composition F.cross_entropy (+ output.max(1)[1]) on the same labels, on any device.  Class weights, label smoothing, probability
    targets and bf16 logits are not supported.  return_pred=True returns (loss, pred int64 [n]).  No atomics: two runs are bit-equal."""
    if reduction not in ("mean", "sum"):
        raise ValueError("cross_entropy: reduction must be 'mean' or 'sum'")
    fused = FUSED_DEFAULT if fused is None else bool(fused)
    if not (torch.is_tensor(output) and output.dim() == 2 and output.shape[1] >= 1):
        raise TypeError("cross_entropy: output must be a [n, C >= 1] matrix of logits")
    if fused:
        dev._no_bf16("cross_entropy", output)
        dev._check_mat(output, "output")
    n, c = output.shape
    y, live = _class_labels(labels, c, n, output.device, ignore_index, check)
    if not fused:
        loss = F.cross_entropy(output, torch.where(y < 0, torch.full_like(y, -100), y), reduction=reduction, ignore_index=-100)
        return (loss, output.detach().max(1)[1]) if return_pred else loss
    w, scale = 1.0, None
    if reduction == "mean":
        if check:
            w = 1.0 / live if live else float("nan")
        else:
            scale = 1.0 / live.to(torch.float64)
    if torch.is_grad_enabled() and output.requires_grad:
        loss, pred = _CrossEntropy.apply(output, y, w, scale, bool(return_pred))
    else:
        _, row_loss, pred = dev.class_loss_grad(output.detach(), y, w, row_loss=True, pred=bool(return_pred))
        loss = (row_loss.sum(dtype=torch.float64) * (w if scale is None else scale)).to(torch.float32)
    return (loss, pred) if return_pred else loss


def loge_cross_entropy(output, labels, epsilon=LOGE_EPSILON, **kw):
    """LogeCrossEntropy of the reference (sgl/tricks/utils.py:7-10) as written: log(epsilon + L) - log(epsilon) with L the MEAN
    cross-entropy -- a scalar transform of the mean loss, not a per-row one.  Scalar torch operations on top of cross_entropy (whose
    keywords are taken, reduction excepted): the factor 1 / (epsilon + L) reaches dLogits through its backward."""
    if kw.get("reduction", "mean") != "mean":
        raise ValueError("loge_cross_entropy: the reference's loss is a function of the mean cross-entropy")
    got = cross_entropy(output, labels, **kw)
    ce, pred = got if kw.get("return_pred") else (got, None)
    loss = torch.log(epsilon + ce) - math.log(epsilon)
    return (loss, pred) if kw.get("return_pred") else loss


def predict(output):
    """output.max(1)[1] of accuracy (sgl/tasks/utils.py:13) for a [n, C] float32 CUDA matrix: the lowest index of every row's maximum,
    int64 [n] -- the launch with one output: one read of the logits, no exp.  A NaN counts as the maximum, the first NaN wins."""
    dev._no_bf16("predict", output)
    dev._check_mat(output, "output")
    return dev.class_loss_grad(output.detach(), None, 1.0, pred=True)[2]


def _pred_of(output):
    """predict for a device matrix; a model output that lives on the host is scored there (output.max(1)[1])"""
    return predict(output) if output.is_cuda else output.detach().max(1)[1]


def _correct(pred, labels):
    return pred.eq(labels.to(pred.device)).double().sum()


def accuracy(output, labels):
    """accuracy of the reference (sgl/tasks/utils.py:12-16): the share of rows whose predict()ed class is the label, a Python float
    (one host read)"""
    labels = _as_index(labels, output.device)
    return (_correct(_pred_of(output), labels) / len(labels)).item()


_BUILT_IN = {"cross_entropy": cross_entropy, "loge": loge_cross_entropy}


def _loss_and_pred(loss_fn, output, y):
    """(loss, pred): one launch for a built-in loss; a callable takes the unfused route -- its own loss, pred from predict"""
    if isinstance(loss_fn, str):
        if loss_fn not in _BUILT_IN:
            raise ValueError(f"loss_fn must be one of {sorted(_BUILT_IN)} or a callable, not {loss_fn!r}")
        return _BUILT_IN[loss_fn](output, y, check=False, return_pred=True)
    if not callable(loss_fn):
        raise TypeError("loss_fn must be 'cross_entropy', 'loge' or a callable")
    return loss_fn(output, y), _pred_of(output)


def _check_loss_fn(loss_fn):
    if isinstance(loss_fn, str) and loss_fn not in _BUILT_IN:
        raise ValueError(f"loss_fn must be one of {sorted(_BUILT_IN)} or a callable, not {loss_fn!r}")
    if not isinstance(loss_fn, str) and not callable(loss_fn):
        raise TypeError("loss_fn must be 'cross_entropy', 'loge' or a callable")


def train(model, train_idx, labels, device, optimizer, loss_fn="cross_entropy"):
    """train of the reference (sgl/tasks/utils.py:66-76), one full-batch step: model_forward, the loss and the accuracy of the output,
    backward, optimizer.step.  labels: the int64 labels of ALL nodes on `device`.  With a built-in loss one launch gives the loss,
    dLogits and the predictions.  Returns (loss, acc) as Python floats: one host read for both."""
    _check_loss_fn(loss_fn)
    device = torch.device(device)
    model.train()
    optimizer.zero_grad()
    y = labels[_as_index(train_idx, labels.device)]
    output = model.model_forward(train_idx, device)
    loss, pred = _loss_and_pred(loss_fn, output, y)
    correct = _correct(pred, y)
    loss.backward()
    optimizer.step()
    loss_v, correct_v = torch.stack((loss.detach().double(), correct.to(loss.device))).tolist()
    return loss_v, correct_v / len(y)


def mini_batch_train(model, train_idx, train_loader, labels, device, optimizer, loss_fn="cross_entropy"):
    """mini_batch_train of the reference (sgl/tasks/utils.py:79-98): one step per batch of `train_loader` (an iterable of index
    batches); the loss is the unweighted mean of the batch losses, the accuracy the correct count over len(train_idx).  One host read
    at the end of the epoch."""
    _check_loss_fn(loss_fn)
    device = torch.device(device)
    model.train()
    losses, correct = [], None
    for batch in train_loader:
        y = labels[_as_index(batch, labels.device)]
        output = model.model_forward(batch, device)
        loss, pred = _loss_and_pred(loss_fn, output, y)
        hit = _correct(pred, y)
        correct = hit if correct is None else correct + hit
        losses.append(loss.detach().double())
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
    if not losses:
        raise ValueError("mini_batch_train: the loader yielded no batch")
    values = torch.stack(losses + [correct.to(losses[0].device)]).tolist()
    return sum(values[:-1]) / len(losses), values[-1] / len(train_idx)


def _forward_pred(model, idx, device):
    return _pred_of(model.model_forward(idx, device))


@torch.no_grad()
def evaluate(model, val_idx, test_idx, labels, device):
    """evaluate of the reference (sgl/tasks/utils.py:38-45): (acc_val, acc_test) of the model in eval mode -- two arg-max launches,
    one host read for both accuracies"""
    device = torch.device(device)
    model.eval()
    counts = [_correct(_forward_pred(model, idx, device), labels[_as_index(idx, labels.device)]) for idx in (val_idx, test_idx)]
    val, test = torch.stack(counts).tolist()
    return val / len(val_idx), test / len(test_idx)


@torch.no_grad()
def mini_batch_evaluate(model, val_idx, val_loader, test_idx, test_loader, labels, device):
    """mini_batch_evaluate of the reference (sgl/tasks/utils.py:48-63): the correct counts of the batches over len(val_idx) and
    len(test_idx); one host read"""
    device = torch.device(device)
    model.eval()
    counts = []
    for loader in (val_loader, test_loader):
        total = torch.zeros((), dtype=torch.float64, device=labels.device)
        for batch in loader:
            total = total + _correct(_forward_pred(model, batch, device), labels[_as_index(batch, labels.device)]).to(labels.device)
        counts.append(total)
    val, test = torch.stack(counts).tolist()
    return val / len(val_idx), test / len(test_idx)


def epoch_batches(idx, batch_size, seed=None, device="cpu"):
    """`idx` (int64 tensor on `device`) cut into batches of `batch_size` (the last one shorter: drop_last=False); seed=None keeps the
    order (the evaluation loaders), otherwise the order is a permutation drawn on `device` from a generator seeded with `seed` (the
    training loader: node_classification passes seed + epoch).  The same seed gives the same batches."""
    if batch_size is None or int(batch_size) < 1:
        raise ValueError("batch_size must be a positive integer")
    idx = _as_index(idx, device)
    if seed is not None:
        gen = torch.Generator(device=idx.device)
        gen.manual_seed(int(seed))
        idx = idx[torch.randperm(idx.numel(), generator=gen, device=idx.device)]
    return list(idx.split(int(batch_size)))


NodeClassificationResult = namedtuple("NodeClassificationResult", ["best_val", "best_test", "history"])
NodeClassificationResult.__doc__ = """node_classification's result: the validation accuracy NodeClassification keeps and the test accuracy
that came with it (its test_acc), and history = one dict per epoch (epoch, loss, acc_train, acc_val, acc_test) followed by the
post-processing entry (epoch = "post", acc_val, acc_test)"""


def node_classification(model, adj, x, y, train_idx, val_idx, test_idx, epochs, lr, weight_decay, loss_fn="cross_entropy", seed=42,
                        train_batch_size=None, eval_batch_size=None, batches=None, device="cuda"):
    """NodeClassification._execute and _postprocess of the reference (sgl/tasks/node_classification.py:45-112), on the device:
    torch.manual_seed(seed), model.preprocess(adj, x), Adam(lr, weight_decay), `epochs` times train + evaluate (mini_batch_train +
    mini_batch_evaluate when train_batch_size is given), then the post-processing step -- model_forward over all nodes in eval mode
    -> model.postprocess(adj, output) when the model has one -> the two accuracies.  A strictly greater validation accuracy takes its
    test accuracy with it; the bests start at 0.  Returns a NodeClassificationResult.
    loss_fn: "cross_entropy", "loge" or a callable (output, labels) -> scalar.  Mini-batches: the training batches of epoch e are a
    permutation drawn on the device from a generator seeded with seed + e (the reference's DataLoader shuffles from the global torch
    generator); the evaluation batches keep their order.  batches: a dict that overrides them with explicit lists of index batches --
    "train" (used every epoch; or a callable epoch -> list), "val", "test", "all".
    The reference passes a torch `x` to preprocess, which its own propagate rejects; here both ndarray and tensor are accepted, as
    everywhere else."""
    _check_loss_fn(loss_fn)
    device = torch.device(device)
    y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).reshape(-1).to(device=device, dtype=torch.int64)
    n = int(y.numel())
    batches = dict(batches or {})
    unknown = set(batches) - {"train", "val", "test", "all"}
    if unknown:
        raise ValueError(f"batches: unknown keys {sorted(unknown)}")
    mini = train_batch_size is not None or "train" in batches
    if mini and eval_batch_size is None and not {"val", "test", "all"} <= set(batches):
        raise ValueError("node_classification: mini-batch training needs eval_batch_size (or explicit val / test / all batches)")
    torch.manual_seed(seed)
    model.preprocess(adj, x)
    model = model.to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    if mini:
        ordered = {key: batches[key] if key in batches else epoch_batches(idx, eval_batch_size, None, device)
                   for key, idx in (("val", val_idx), ("test", test_idx), ("all", range(n)))}
    best_val, best_test = 0., 0.
    history = []
    for epoch in range(epochs):
        if not mini:
            loss, acc = train(model, train_idx, y, device, optimizer, loss_fn)
            acc_val, acc_test = evaluate(model, val_idx, test_idx, y, device)
        else:
            if "train" in batches:
                loader = batches["train"](epoch) if callable(batches["train"]) else batches["train"]
            else:
                loader = epoch_batches(train_idx, train_batch_size, seed + epoch, device)
            loss, acc = mini_batch_train(model, train_idx, loader, y, device, optimizer, loss_fn)
            acc_val, acc_test = mini_batch_evaluate(model, val_idx, ordered["val"], test_idx, ordered["test"], y, device)
        history.append(dict(epoch=epoch, loss=loss, acc_train=acc, acc_val=acc_val, acc_test=acc_test))
        if acc_val > best_val:
            best_val, best_test = acc_val, acc_test
    with torch.no_grad():                              # _postprocess (lines 93-112)
        model.eval()
        if not mini:
            out = model.model_forward(range(n), device)
        else:
            out = torch.vstack([model.model_forward(batch, device) for batch in ordered["all"]])
        if hasattr(model, "postprocess"):
            out = model.postprocess(adj, out)
        counts = []
        for idx in (val_idx, test_idx):
            at = _as_index(idx, out.device)
            rows = out[at]
            counts.append(_correct(_pred_of(rows), y[at.to(y.device)]))
        val, test = torch.stack(counts).tolist()
    acc_val, acc_test = val / len(val_idx), test / len(test_idx)
    history.append(dict(epoch="post", acc_val=acc_val, acc_test=acc_test))
    if acc_val > best_val:
        best_val, best_test = acc_val, acc_test
    return NodeClassificationResult(best_val, best_test, history)


HeteroNodeClassificationResult = namedtuple("HeteroNodeClassificationResult", ["best_val", "best_test", "subgraph_weight", "history"])
HeteroNodeClassificationResult.__doc__ = """hetero_node_classification's result: the best validation accuracy, the test accuracy that came
with it (HeteroNodeClassification's test_acc), the model's subgraph_weight at that epoch (None unless record_subgraph_weight), and
history = one dict per epoch (epoch, loss, acc_train, acc_val, acc_test)"""


def hetero_node_classification(model, dataset, predict_class, epochs, lr, weight_decay, loss_fn="cross_entropy", seed=42,
                               train_batch_size=None, eval_batch_size=None, random_subgraph_num=-1, subgraph_edge_type_num=-1,
                               subgraph_list=None, record_subgraph_weight=False, device="cuda"):
    """HeteroNodeClassification._execute of the reference (sgl/tasks/node_classification.py:115-217) on the device: torch.manual_seed,
    model.preprocess(dataset, predict_class, ...), Adam, `epochs` times train + evaluate (the mini-batch forms when train_batch_size
    is given; batches as in node_classification), a strictly greater validation accuracy takes its test accuracy -- and, with
    record_subgraph_weight, a copy of model.subgraph_weight -- with it.  The labels are dataset.data[predict_class].y; the index sets
    dataset.train_idx / val_idx / test_idx count inside the predict class.  There is no post-processing step."""
    _check_loss_fn(loss_fn)
    if subgraph_list is None and (random_subgraph_num == -1 or subgraph_edge_type_num == -1):
        raise ValueError("Either subgraph_list or (random_subgraph_num, subgraph_edge_type_num) should be provided!")
    if subgraph_list is not None and (random_subgraph_num != -1 or subgraph_edge_type_num != -1):
        raise ValueError("subgraph_list is provided, random_subgraph_num and subgraph_edge_type_num will be ignored!")
    mini = train_batch_size is not None
    if mini and eval_batch_size is None:
        raise ValueError("hetero_node_classification: mini-batch training needs eval_batch_size")
    device = torch.device(device)
    y = dataset.data[predict_class].y
    y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).reshape(-1).to(device=device, dtype=torch.int64)
    train_idx, val_idx, test_idx = dataset.train_idx, dataset.val_idx, dataset.test_idx
    torch.manual_seed(seed)
    model.preprocess(dataset, predict_class, random_subgraph_num, subgraph_edge_type_num, subgraph_list)
    model = model.to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    if mini:
        val_loader, test_loader = (epoch_batches(idx, eval_batch_size, None, device) for idx in (val_idx, test_idx))
    best_val, best_test, history = 0., 0., []
    best_weight = model.subgraph_weight.detach().clone() if record_subgraph_weight else None
    for epoch in range(epochs):
        if not mini:
            loss, acc = train(model, train_idx, y, device, optimizer, loss_fn)
            acc_val, acc_test = evaluate(model, val_idx, test_idx, y, device)
        else:
            loader = epoch_batches(train_idx, train_batch_size, seed + epoch, device)
            loss, acc = mini_batch_train(model, train_idx, loader, y, device, optimizer, loss_fn)
            acc_val, acc_test = mini_batch_evaluate(model, val_idx, val_loader, test_idx, test_loader, y, device)
        history.append(dict(epoch=epoch, loss=loss, acc_train=acc, acc_val=acc_val, acc_test=acc_test))
        if acc_val > best_val:
            best_val, best_test = acc_val, acc_test
            if record_subgraph_weight:
                best_weight = model.subgraph_weight.detach().clone()
    return HeteroNodeClassificationResult(best_val, best_test, best_weight, history)


class HeteroNodeClassification:
    """the reference's task object: runs on construction, then test_acc and subgraph_weight"""

    def __init__(self, dataset, predict_class, model, lr, weight_decay, epochs, device, loss_fn="cross_entropy", seed=42,
                 train_batch_size=None, eval_batch_size=None, random_subgraph_num=-1, subgraph_edge_type_num=-1, subgraph_list=None,
                 record_subgraph_weight=False):
        self.result = hetero_node_classification(model, dataset, predict_class, epochs, lr, weight_decay, loss_fn=loss_fn, seed=seed,
                                                 train_batch_size=train_batch_size, eval_batch_size=eval_batch_size,
                                                 random_subgraph_num=random_subgraph_num, subgraph_edge_type_num=subgraph_edge_type_num,
                                                 subgraph_list=subgraph_list, record_subgraph_weight=record_subgraph_weight, device=device)

    test_acc = property(lambda self: self.result.best_test)
    subgraph_weight = property(lambda self: self.result.subgraph_weight)

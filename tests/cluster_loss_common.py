"""Shared by test_cluster_loss_cpu.py and test_gpu_cluster_loss.py (importable without a GPU), and by
golden/make_g19_node_clustering_train.py: the inputs of the cluster-loss tests, their CPU references -- CPU autograd of the reference's
own expression (sgl/tasks/utils.py:101-113: one torch.norm per centre, cat, mean(1).sum(), the assigned distances) in float32 and in
float64, computed once per case and left unchanged -- the formulas of csrc/sgl_cluster_loss.hip restated in numpy, and the restated
selection rule of the kernel's instances.

Acceptance is oracle.truth_report(got, ref32, truth, cond=cond) with its defaults: at most twice as far from the float64 truth as the
reference's own float32 result, with the floor of 16 float32 roundings of the largest entry, or of `cond` -- the sum of the ABSOLUTE
contributions to an entry: sum_j |a_ij| |x_i - c_j| / n for dX, sum_ij |w_ij| D_ij / n for the loss (w_ij = 2 [j = y_i] - 1 / k).  No
tolerance is chosen here.  That rule is a condition on the INPUTS: test_cluster_loss_cpu.py checks that the plain float32 numpy
restatement below passes it on every case the GPU test uses."""
import re

import numpy as np
import torch

from edge_scores_common import pick_lpr
from kmeans_common import BIG, N_ROWS, host_centres, host_x
from spmm_order_common import parse_template_args

WIDTHS = (1, 3, 4, 7, 12, 31, 33, 64, 100, 128, 147, 257, 600, 1030, 2500)
KS = (1, 2, 7, 47, 64)
ZERO_CENTRES = 3                                   # up to this many centres are exact copies of rows: zero distances occur
SHIFT = 100.0                                      # the translation of the invariance test, per column
_NAME = re.compile(r"cluster_loss_(stream_)?kernel")


def cases():
    return [(d, k) for d in WIDTHS for k in KS] + list(BIG)


_IN, _REF = {}, {}


def inputs(d, k, shift=0.0, n=N_ROWS):
    """(x [n, d], centres [k, d], labels int64 [n]): kmeans_common's matrices, the first min(3, k) centres overwritten with
    exact copies of seeded rows, labels from a seeded rng; shift: added to every column of x and of the centres IN FLOAT32 (the
    shifted float32 matrices are the inputs of that test: its references are recomputed from them)"""
    key = (d, k, shift, n)
    if key not in _IN:
        rng = np.random.default_rng(90000 + 131 * d + k)
        x, c = host_x(d, n).copy(), host_centres(d, k, n).copy()
        rows = rng.choice(n, min(ZERO_CENTRES, k), replace=False)
        c[:len(rows)] = x[rows]
        y = rng.integers(0, k, n).astype(np.int64)
        if shift:
            x, c = (x + np.float32(shift)).astype(np.float32), (c + np.float32(shift)).astype(np.float32)
        _IN[key] = (x, c, y)
    return _IN[key]


# ---- references: CPU autograd of the reference's expression ----------------------------------------------------------------------------
def reference_loss(out, y, centres, reduction="mean"):
    """cluster_loss as the reference writes it, for torch tensors of any float dtype; the assigned distances are gathered (the
    reference picks them with a Python generator over the rows: the same values and the same autograd gradient)"""
    for i in range(len(centres)):
        col = torch.norm(out - centres[i], p=2, dim=1, keepdim=True)
        dist = col if i == 0 else torch.cat((dist, col), 1)
    loss = -dist.mean(1).sum() + 2 * dist[torch.arange(dist.shape[0]), y].sum()
    return loss / dist.shape[0] if reduction == "mean" else loss


def step_references(x, centres, y, reduction="mean"):
    """{"ref32" | "truth" | "cond": (loss, dX)}"""
    out = {}
    yt = torch.from_numpy(np.asarray(y, dtype=np.int64))
    for name, dt in (("ref32", torch.float32), ("truth", torch.float64)):
        xx = torch.from_numpy(np.ascontiguousarray(x)).to(dt).requires_grad_(True)
        loss = reference_loss(xx, yt, torch.from_numpy(np.ascontiguousarray(centres)).to(dt), reduction)
        loss.backward()
        out[name] = (float(loss.detach()), xx.grad.numpy())
    x64, c64 = np.asarray(x, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    n, k = x64.shape[0], c64.shape[0]
    scale = 1.0 / n if reduction == "mean" else 1.0
    cond_loss, cond_dx = 0.0, np.zeros_like(x64)
    for j in range(k):
        diff = x64 - c64[j]
        dist = np.sqrt((diff ** 2).sum(1))
        wgt = np.abs(2.0 * (y == j) - 1.0 / k)
        cond_loss += float((wgt * dist).sum())
        a = np.divide(wgt, dist, out=np.zeros_like(dist), where=dist > 0)
        cond_dx += a[:, None] * np.abs(diff)
    out["cond"] = (cond_loss * scale, cond_dx * scale)
    return out


def references(d, k, shift=0.0):
    """step_references of inputs(d, k, shift); computed once"""
    key = (d, k, shift)
    if key not in _REF:
        _REF[key] = step_references(*inputs(d, k, shift))
    return _REF[key]


# ---- the kernel's formulas, restated in numpy (any float dtype: the dtype of x) ----------------------------------------------------------
def restated_rows(x, centres, y, w):
    """(row_loss [n], dX [n, d]) by the formulas of csrc/sgl_cluster_loss.hip in x's dtype, centre after centre: D = sqrt(sum (x - c)^2),
    a = (2 [j = y] - 1 / k) / D and 0 where D = 0, dX += a (x - c); l = 2 D_y - (sum D) (1 / k); dX scaled by w at the end.  A label
    outside [0, k) matches no centre.  (The kernel adds the D of a row as four partial sums, centres j = t mod 4 each: a restatement of
    the formulas, not of the bits.)"""
    x = np.asarray(x)
    dt = x.dtype.type
    c = np.asarray(centres, dtype=x.dtype)
    n, k = x.shape[0], c.shape[0]
    inv_k = dt(np.float32(1.0) / np.float32(k)) if x.dtype == np.float32 else dt(1.0) / dt(k)
    total, mine, dx = np.zeros(n, dtype=x.dtype), np.zeros(n, dtype=x.dtype), np.zeros_like(x)
    for j in range(k):
        diff = x - c[j]
        dist = np.sqrt((diff * diff).sum(1, dtype=x.dtype))
        hit = np.asarray(y) == j
        wgt = np.where(hit, dt(2), dt(0)) - inv_k
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(dist == 0, dt(0), wgt / dist)
        total += dist
        mine = np.where(hit, dist, mine)
        dx += a[:, None] * diff
    return dt(2) * mine - total * inv_k, dx * dt(w)


def restated_step(x, centres, y, reduction="mean"):
    """(loss, dX): the float64 sum of the restated row losses times w, and the restated dX"""
    w = 1.0 / len(x) if (reduction == "mean" and len(x)) else 1.0
    rows, dx = restated_rows(x, centres, y, w)
    return float(rows.astype(np.float64).sum() * w), dx


# ---- the instance rule of sgl_cluster_loss_grad_f32 --------------------------------------------------------------------------------------
def _vectored(t):
    pitch = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
    return t.data_ptr() % 16 == 0 and pitch % 4 == 0


def rows_per_group(vec, ch):
    return 4 if vec * ch * 8 <= 64 else (2 if vec * ch * 4 <= 64 else 1)


def expected_instance(x, centres, dx=None):
    """(LPR, VEC, CH, U): 16-byte lanes iff the bases of x, the centres and (when given) dX are 16-byte aligned and their pitches
    multiples of 4 floats (a one-row matrix is passed with pitch d); LPR from the width and the lane size; CH = vectors per lane of
    the compiled instance -- 1 with any lane count, then 64 lanes with 2 / 4 / 8 vectors (VEC = 4) or 2 / 8 / 32 floats (VEC = 1);
    U = rows per lane group.  Beyond: the streaming kernel, (64, VEC, 0, 1)"""
    d = x.shape[1]
    vec = 4 if all(_vectored(t) for t in (x, centres, dx) if t is not None) else 1
    lpr = pick_lpr(d, vec)
    chunks = -(-d // (lpr * vec))
    steps = (2, 4, 8) if vec == 4 else (2, 8, 32)
    ch = 1 if chunks == 1 else next((c for c in steps if chunks <= c), 0)
    if ch == 0:
        return (64, vec, 0, 1)
    return (lpr, vec, ch, rows_per_group(vec, ch))


def compiled_instances():
    out = set()
    for vec, steps in ((4, (2, 4, 8)), (1, (2, 8, 32))):
        out |= {(lpr, vec, 1, rows_per_group(vec, 1)) for lpr in (8, 16, 32, 64)}
        out |= {(64, vec, c, rows_per_group(vec, c)) for c in steps}
        out.add((64, vec, 0, 1))
    return out


def parse_kernel_name(name):
    """(LPR, VEC, CH, U) from the name of a cluster_loss_kernel instance, (64, VEC, 0, 1) from a cluster_loss_stream_kernel one, None
    for any other kernel"""
    m = _NAME.search(name)
    if not m:
        return None
    args = parse_template_args(name[m.end():])
    if args is None or len(args) != (1 if m.group(1) else 4):
        raise ValueError(f"unexpected template arguments in {name!r}")
    return (64, args[0], 0, 1) if m.group(1) else tuple(args)

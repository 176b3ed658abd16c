"""Shared by test_class_loss_cpu.py and test_gpu_class_loss.py (importable without a GPU): the inputs of the class-loss tests, their
CPU references -- F.cross_entropy (mean over the labelled rows, ignore_index = -100) under CPU autograd in float32 and in float64,
computed once per width and left unchanged -- the formulas of csrc/sgl_class_loss.hip restated in numpy, the arg-max cases, and the
restated selection rule of the kernel's instances.

Acceptance is oracle.truth_report(got, ref32, truth, cond=cond) with its defaults: at most twice as far from the float64 truth as the
reference's own float32 result, with the floor of 16 float32 roundings of the largest entry, or of `cond` -- the sum of the ABSOLUTE
contributions to an entry: (p + onehot) / live for dZ, sum_live (|lse_i| + |z_{i, y_i}|) / live for the loss.  No tolerance is chosen
here.  That rule is a condition on the INPUTS: test_class_loss_cpu.py checks that the plain float32 numpy restatement below passes it
at every width the GPU test uses."""
import re

import numpy as np
import torch
import torch.nn.functional as F

from edge_scores_common import pick_lpr
from spmm_order_common import parse_template_args

N_ROWS = 1031
# the widths that exist (3, 7, 40 / 47, 172), the edges of every lane layout, and the two sides of the register / stream boundary
# (1024 | 1025); 12 is the one width that takes 16 lanes of one float
WIDTHS = (1, 2, 3, 4, 7, 12, 31, 33, 47, 64, 100, 172, 257, 600, 1024, 1025, 1030, 2500)
IGNORE = -100
IGNORE_EVERY = 17
_NAME = re.compile(r"class_loss_(stream_)?kernel")

_IN, _REF = {}, {}


def inputs(c, n=N_ROWS):
    """(z float32 [n, c], labels int64 [n]): per row a scale from (0.1, 1, 8, 40) and an offset from (0, 0, 1e4, -3e3) around standard
    normal noise; labels uniform in [0, c) with every 17th row -100"""
    if (c, n) not in _IN:
        rng = np.random.default_rng(70000 + c)
        z = (rng.standard_normal((n, c)) * rng.choice([0.1, 1.0, 8.0, 40.0], (n, 1)) + rng.choice([0.0, 0.0, 1e4, -3e3], (n, 1))).astype(np.float32)
        y = rng.integers(0, c, n).astype(np.int64)
        y[::IGNORE_EVERY] = IGNORE
        _IN[(c, n)] = (z, y)
    return _IN[(c, n)]


# ---- references: CPU autograd of F.cross_entropy -------------------------------------------------------------------------------------------
def step_references(z, y, reduction="mean"):
    """{"ref32" | "truth" | "cond": (loss, dZ)} of F.cross_entropy(z, y, ignore_index=-100)"""
    out = {}
    yt = torch.from_numpy(np.asarray(y, dtype=np.int64))
    for name, dt in (("ref32", torch.float32), ("truth", torch.float64)):
        zz = torch.from_numpy(np.ascontiguousarray(z)).to(dt).requires_grad_(True)
        loss = F.cross_entropy(zz, yt, reduction=reduction, ignore_index=IGNORE)
        loss.backward()
        out[name] = (float(loss.detach()), zz.grad.numpy())
    z64 = np.asarray(z, dtype=np.float64)
    n, c = z64.shape
    live = (np.asarray(y) >= 0) & (np.asarray(y) < c)
    scale = 1.0 / max(int(live.sum()), 1) if reduction == "mean" else 1.0
    m = z64.max(1, keepdims=True)
    e = np.exp(z64 - m)
    s = e.sum(1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    onehot = np.zeros_like(z64)
    rows = np.flatnonzero(live)
    onehot[rows, np.asarray(y)[rows]] = 1.0
    zy = np.where(live, z64[np.arange(n), np.where(live, y, 0)], 0.0)
    out["cond"] = (float(((np.abs(lse) + np.abs(zy)) * live).sum() * scale), (e / s + onehot) * live[:, None] * scale)
    return out


def references(c):
    """step_references of inputs(c); computed once"""
    if c not in _REF:
        _REF[c] = step_references(*inputs(c))
    return _REF[c]


def weight(y, c):
    """1 / (number of rows with a label in [0, c)), the w of the mean"""
    live = int(((np.asarray(y) >= 0) & (np.asarray(y) < c)).sum())
    return 1.0 / live if live else 1.0


# ---- the kernel's formulas, restated in numpy (any float dtype: the dtype of z) ---------------------------------------------------------
def restated_rows(z, y, w):
    """(row_loss [n], dZ [n, c], pred [n]) by the formulas of csrc/sgl_class_loss.hip in z's dtype: m = max, e = exp(z - m), s = sum e
    (in that dtype), lse = m + log s, l = lse - z_y, dZ = w (e / s - onehot); 0 for a row whose label is outside [0, c); pred = the
    first index of the maximum, a NaN counting as the maximum.  A restatement of the formulas, not of the bits (the kernel adds the
    exponentials lane by lane)."""
    z = np.asarray(z)
    dt = z.dtype.type
    n, c = z.shape
    y = np.asarray(y)
    live = (y >= 0) & (y < c)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.fmax.reduce(z, axis=1, keepdims=True) if c else np.zeros((n, 1), z.dtype)
        e = np.exp(z - m)
        s = e.sum(1, dtype=z.dtype, keepdims=True)
        lse = (m + np.log(s))[:, 0]
        safe = np.where(live, y, 0)
        onehot = np.zeros_like(z)
        onehot[np.arange(n), safe] = 1
        rows = np.where(live, lse - z[np.arange(n), safe], dt(0))
        dz = np.where(live[:, None], dt(w) * (e / s - onehot), dt(0))
    return rows.astype(z.dtype), dz.astype(z.dtype), reference_pred(z)


def restated_step(z, y, reduction="mean"):
    """(loss, dZ): the float64 sum of the restated row losses times w, and the restated dZ"""
    w = weight(y, np.asarray(z).shape[1]) if reduction == "mean" else 1.0
    rows, dz, _ = restated_rows(z, y, w)
    return float(rows.astype(np.float64).sum() * w), dz


def reference_pred(z):
    """output.max(1)[1] on the CPU: the first index of the maximum; a NaN is the maximum and the first NaN wins"""
    return torch.from_numpy(np.ascontiguousarray(z)).max(1)[1].numpy()


def unique_maximum(z):
    """the rows whose float32 maximum is held by one entry: their arg-max is a property of the input, not of an order"""
    return (z == z.max(1, keepdims=True)).sum(1) == 1


def argmax_cases(c, n=64):
    """[n, c] float32 rows with constructed arg-max cases (c >= 3): rows 0 .. 3 of every 8 hold an exact tie of two, an exact tie of
    three, one NaN below the maximum's column or above it, and two NaNs; the rest are random with distinct entries"""
    rng = np.random.default_rng(71000 + c)
    z = rng.permutation(n * c).reshape(n, c).astype(np.float32) / np.float32(8.0)     # distinct within and across rows
    for i in range(0, n, 8):
        cols = rng.choice(c, 3, replace=False)
        top = np.float32(z[i].max() + 1.0)
        z[i, cols[:2]] = top                                                         # two equal maxima
        top = np.float32(z[i + 1].max() + 1.0)
        z[i + 1, cols] = top                                                         # three
        z[i + 2, cols[0]] = np.nan                                                   # a NaN wherever the maximum is
        z[i + 3, cols[1:]] = np.nan                                                  # two NaNs: the first one wins
    return z


# ---- the instance rule of sgl_class_loss_grad_f32 ----------------------------------------------------------------------------------------
CHUNKS = {4: (2, 4), 1: (2, 4, 8, 16)}            # vectors per lane of the compiled 64-lane instances, per lane size


def _vectored(t):
    pitch = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
    return t.data_ptr() % 16 == 0 and pitch % 4 == 0


def instance_for(c, vec):
    """sgl::class_loss_instance (csrc/sgl_core.cpp) -> (LPR, VEC, CH): the narrowest lane group that covers the row with one vector per
    lane, then 64 lanes with the next compiled number of vectors, then the streaming kernel (64, VEC, 0)"""
    lpr = pick_lpr(c, vec)
    chunks = -(-c // (lpr * vec))
    ch = 1 if chunks == 1 else next((k for k in CHUNKS[vec] if chunks <= k), 0)
    return (64, vec, 0) if ch == 0 else (lpr, vec, ch)


def expected_instance(z, dz=None):
    """(LPR, VEC, CH): 16-byte lanes iff the bases of z and (when given) dZ are 16-byte aligned and their pitches multiples of 4 floats
    (a one-row matrix is passed with pitch c)"""
    vec = 4 if all(_vectored(t) for t in (z, dz) if t is not None) else 1
    return instance_for(z.shape[1], vec)


def compiled_instances():
    out = set()
    for vec, steps in CHUNKS.items():
        out |= {(lpr, vec, 1) for lpr in (8, 16, 32, 64)}
        out |= {(64, vec, k) for k in steps}
        out.add((64, vec, 0))
    return out


def rows_per_group(vec, ch):
    """U of class_loss_kernel<LPR, VEC, CH, U>: the rows a lane group loads before it reduces the first, as many as keep the slices
    within 16 registers, at most 8"""
    return 1 if vec * ch >= 16 else min(8, 16 // (vec * ch))


def parse_kernel_name(name):
    """(LPR, VEC, CH) from the name of a class_loss_kernel<LPR, VEC, CH, U> instance (U must be rows_per_group(VEC, CH)), (64, VEC, 0)
    from a class_loss_stream_kernel one, None for any other kernel"""
    m = _NAME.search(name)
    if not m:
        return None
    args = parse_template_args(name[m.end():])
    if args is None or len(args) != (1 if m.group(1) else 4):
        raise ValueError(f"unexpected template arguments in {name!r}")
    if m.group(1):
        return (64, args[0], 0)
    if args[3] != rows_per_group(args[1], args[2]):
        raise ValueError(f"unexpected rows per group in {name!r}")
    return tuple(args[:3])

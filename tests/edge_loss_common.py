"""Shared by test_edge_loss_cpu.py and test_gpu_edge_loss.py (importable without a GPU): a numpy restatement of EdgePlan's tables, the
formulas of csrc/sgl_edge_loss.hip restated in numpy, the CPU references of loss and dZ -- CPU autograd of the reference's own
expression, torch.mm(Z, Z.t())[e0, e1] -> sigmoid -> binary_cross_entropy_with_logits (sgl/tasks/utils.py:281-293), in float32 and
float64, computed once per case and left unchanged -- and the restated selection rule of the kernel's instances."""
import re

import numpy as np
import torch
import torch.nn.functional as F

from edge_scores_common import EDGES, N_EDGES, N_ROWS, host_matrix, pick_lpr
from inputs import hash_matrix
from spmm_order_common import parse_template_args

KERNEL = "edge_loss_grad_kernel"
_NAME = re.compile(KERNEL)
MODES = {"sigmoid": 0, "none": 1, "given": 2}
# the widths the values are checked at: (1, 3, 7, 100, 128, 147, 257, 600, 1030), and four more so that EVERY compiled instance runs --
# 12, 31, 40 reach the 16- and 32-lane layouts of both lane sizes, 2100 the instance for rows beyond the register layouts
WIDTHS = (1, 3, 7, 12, 31, 40, 100, 128, 147, 257, 600, 1030, 2100)
HUB_NODE, HUB_EDGES = 5, 300


def labels_for(n_edges=N_EDGES):
    """float32 [E]: hard labels for the first four fifths (about half of them 1), soft labels in [0, 1) for the rest"""
    h = hash_matrix(1, n_edges, seed=4242)[0]
    y = (h > 0).astype(np.float32)
    soft = n_edges - n_edges // 5
    y[soft:] = (h[soft:] + 1.0) / 2.0
    return y


LABELS = labels_for()


def hub_edges(n=N_ROWS):
    """[300, 2]: every edge has node 5 at one end (alternating sides), one of them a self pair; nodes >= 200 stay isolated"""
    other = (np.arange(HUB_EDGES, dtype=np.int64) * 7) % 200
    e = np.stack((np.full(HUB_EDGES, HUB_NODE, dtype=np.int64), other), axis=1)
    e[1::2] = e[1::2, ::-1]
    e[10] = (HUB_NODE, HUB_NODE)
    return e


# ---- the plan's tables, restated with loops -------------------------------------------------------------------------------------------
def plan_tables(edges, n, max_piece):
    """(inc_ptr, inc_other, inc_edge, pieces [P, 4], fold [F, 3], n_partial) as EdgePlan documents them"""
    e = np.asarray(edges, dtype=np.int64)
    if e.size and (e.min() < -n or e.max() >= n):
        raise IndexError("index out of range in edge list")
    e = np.where(e < 0, e + n, e)
    rows = [[] for _ in range(n)]
    for k, (u, v) in enumerate(e):
        rows[u].append((v, k))                       # the primary entry: this row is u_e
        rows[v].append((u, ~k))                      # a self pair: both entries in one row, primary first
    inc_ptr = np.zeros(n + 1, dtype=np.int64)
    other, code, pieces, fold = [], [], [], []
    n_partial = 0
    for i, r in enumerate(rows):
        begin = len(other)
        other += [o for o, _ in r]
        code += [c for _, c in r]
        inc_ptr[i + 1] = len(other)
        cuts = list(range(begin, len(other), max_piece)) or [begin]
        if len(cuts) > 1:
            fold.append((i, n_partial, len(cuts)))
        for b in cuts:
            dest = -1
            if len(cuts) > 1:
                dest = n_partial
                n_partial += 1
            pieces.append((i, b, min(b + max_piece, len(other)), dest))
    return (inc_ptr, np.array(other, dtype=np.int32), np.array(code, dtype=np.int64), np.array(pieces, dtype=np.int64).reshape(-1, 4),
            np.array(fold, dtype=np.int64).reshape(-1, 3), n_partial)


# ---- the kernel's formulas, restated in numpy (any float dtype: the dtype of s) ----------------------------------------------------------
def loss_and_coef(s, y, w, mode):
    """(L, c) per edge as csrc/sgl_edge_loss.hip forms them from e = exp(-|s|)"""
    s = np.asarray(s)
    dt = s.dtype.type
    y = np.asarray(y, dtype=s.dtype)
    e = np.exp(-np.abs(s))
    r = dt(1) / (dt(1) + e)
    sig = np.where(s >= 0, r, e * r)
    if mode == "sigmoid":
        ep = np.exp(-sig)
        return (dt(1) - y) * sig + np.log1p(ep), dt(w) * (dt(1) / (dt(1) + ep) - y) * (e * r * r)
    return np.maximum(s, dt(0)) - s * y + np.log1p(e), dt(w) * np.where(s >= 0, (dt(1) - y) - e * r, sig - y)


def restated_step(z, edges, labels, mode, reduction="mean"):
    """(loss, dZ) of one step by the restated formulas in z's dtype: scores, coefficients, and dZ[i] = sum of c z_j over both ends"""
    z = np.asarray(z)
    e = np.asarray(edges, dtype=np.int64)
    e = np.where(e < 0, e + z.shape[0], e)
    w = 1.0 / len(e) if reduction == "mean" else 1.0
    s = (z[e[:, 0]] * z[e[:, 1]]).sum(1, dtype=z.dtype)
    L, c = loss_and_coef(s, labels, w, mode)
    dz = np.zeros_like(z)
    np.add.at(dz, e[:, 0], c[:, None] * z[e[:, 1]])
    np.add.at(dz, e[:, 1], c[:, None] * z[e[:, 0]])
    return float(L.astype(np.float64).sum() * w), dz


# ---- references: CPU autograd of the reference's expression ---------------------------------------------------------------------------
def step_references(z, edges, labels, mode, reduction="mean"):
    """{"ref32" | "truth" | "cond": (loss, dZ)}: the reference in float32, in float64, and the sums of the absolute contributions --
    the loss's terms are all >= 0, so its cond is the loss itself; dZ's is the same autograd on |Z| with the float64 coefficients'
    magnitudes as the upstream gradient (gradient_references' pattern)"""
    e = torch.from_numpy(np.where(np.asarray(edges) < 0, np.asarray(edges) + z.shape[0], np.asarray(edges)).astype(np.int64))
    out = {}
    coef = None
    for name, dt in (("ref32", torch.float32), ("truth", torch.float64)):
        zz = torch.from_numpy(np.ascontiguousarray(z)).to(dt).requires_grad_(True)
        sim = torch.mm(zz, zz.t())[e[:, 0], e[:, 1]].reshape(-1)
        sim.retain_grad()
        pred = torch.sigmoid(sim) if mode == "sigmoid" else sim
        loss = F.binary_cross_entropy_with_logits(pred, torch.from_numpy(np.asarray(labels)).to(dt), reduction=reduction)
        loss.backward()
        out[name] = (float(loss.detach()), zz.grad.numpy())
        coef = sim.grad.detach()
    za = torch.from_numpy(np.ascontiguousarray(z)).double().abs().requires_grad_(True)
    (torch.mm(za, za.t())[e[:, 0], e[:, 1]].reshape(-1) * coef.abs()).sum().backward()
    out["cond"] = (out["truth"][0], za.grad.numpy())
    return out


_REF = {}


def references(d, mode, which="edges", reduction="mean"):
    """step_references for Z = host_matrix(d) and the shared edge list (`which`: "edges" = EDGES with LABELS, "hub" = hub_edges with
    the first 300 labels); computed once"""
    key = (d, mode, which, reduction)
    if key not in _REF:
        edges, labels = (EDGES, LABELS) if which == "edges" else (hub_edges(), LABELS[:HUB_EDGES])
        _REF[key] = step_references(host_matrix(d), edges, labels, mode, reduction)
    return _REF[key]


# ---- the instance rule of sgl_edge_loss_grad_f32 -------------------------------------------------------------------------------------------
def expected_instance(z, mode):
    """(LPR, VEC, MODE, CH): 16-byte lanes iff z's base is 16-byte aligned and its pitch a multiple of 4 floats; LPR from the width
    and the lane size; CH = vectors per lane of the compiled instance -- 1 with any lane count, then 64 lanes with 2 / 4 / 8 vectors
    (VEC = 4) or 2 / 8 / 32 floats (VEC = 1), and 0 (z_i re-read per chunk) beyond"""
    d = z.shape[1]
    pitch = z.stride(0) if z.shape[0] > 1 else max(d, 1)
    vec = 4 if z.data_ptr() % 16 == 0 and pitch % 4 == 0 else 1
    lpr = pick_lpr(d, vec)
    chunks = -(-d // (lpr * vec))
    steps = (2, 4, 8) if vec == 4 else (2, 8, 32)
    ch = 1 if chunks == 1 else next((c for c in steps if chunks <= c), 0)
    return (lpr, vec, MODES[mode], ch)


def compiled_instances():
    out = set()
    for mode in MODES.values():
        for vec, steps in ((4, (0, 2, 4, 8)), (1, (0, 2, 8, 32))):
            out |= {(lpr, vec, mode, 1) for lpr in (8, 16, 32, 64)} | {(64, vec, mode, c) for c in steps}
    return out


def parse_kernel_name(name):
    """(LPR, VEC, MODE, CH) from the name of an edge_loss_grad_kernel instance, None for any other kernel"""
    m = _NAME.search(name)
    if not m:
        return None
    args = parse_template_args(name[m.end():])
    if args is None or len(args) != 4:
        raise ValueError(f"unexpected template arguments in {name!r}")
    return tuple(args)

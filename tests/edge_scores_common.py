"""Shared by test_gpu_edge_scores.py (and importable without a GPU): the edge list and matrices of the edge-score tests, their CPU
references -- computed once per width and left unchanged -- and the restated selection rule of csrc/sgl_edge.hip's instances."""
import re

import numpy as np
import torch

from inputs import hash_matrix
from spmm_order_common import parse_template_args

N_ROWS = 257
N_EDGES = 1000                     # no multiple of any edges-per-workgroup (16 ... 128)
EDGES_PER_GROUP = 4                # kEdgesPerGroup
WIDTHS = (1, 3, 4, 7, 12, 16, 31, 32, 33, 64, 100, 128, 147, 256, 257, 500, 600, 1030)
KERNEL = "edge_dot_kernel"
_NAME = re.compile(KERNEL)


def pick_lpr(d, vec):
    """sgl::pick_lpr (csrc/sgl_core.cpp): the smallest of 8 / 16 / 32 / 64 lanes that covers ceil(d / vec) lane accesses (64 when none does)"""
    lanes = (d + vec - 1) // vec
    lpr = 8
    while lpr < lanes and lpr < 64:
        lpr <<= 1
    return lpr


def expected_instance(a, b):
    """(LPR, VEC, U) sgl_edge_dot_f32 launches for these two matrices: 16-byte lanes iff both bases are 16-byte aligned and both
    pitches multiples of 4 floats (a one-row matrix is passed with pitch d), LPR from the width and the lane size"""
    d = a.shape[1]

    def pitch(t):
        return t.stride(0) if t.shape[0] > 1 else max(d, 1)

    vec = 4 if all(t.data_ptr() % 16 == 0 and pitch(t) % 4 == 0 for t in (a, b)) else 1
    return (pick_lpr(d, vec), vec, EDGES_PER_GROUP)


def compiled_instances():
    return {(lpr, vec, EDGES_PER_GROUP) for lpr in (8, 16, 32, 64) for vec in (4, 1)}


def parse_edge_kernel_name(name):
    """(LPR, VEC, U) from the name of an edge_dot_kernel instance (demangled or mangled), None for any other kernel"""
    m = _NAME.search(name)
    if not m:
        return None
    args = parse_template_args(name[m.end():])
    if args is None or len(args) != 3:
        raise ValueError(f"unexpected template arguments in {name!r}")
    return tuple(args)


# ---- the edge list --------------------------------------------------------------------------------------------------------------------
DUP = (slice(600, 700), slice(0, 100))           # edges 600..699 repeat edges 0..99
REV = (slice(700, 800), slice(100, 200))         # edges 700..799 are edges 100..199 reversed
SELF = slice(800, 900)                           # (i, i)
NEG = (slice(900, 1000), slice(200, 300))        # edges 900..999 are edges 200..299 written with negative indices


def edge_list(n=N_ROWS):
    """[1000, 2] int64: 600 seeded random pairs (the first ones touch the last row, whose pitch the storage need not hold), then
    duplicates, reversed twins, self pairs and negative-index twins of them"""
    rng = np.random.default_rng(2024)
    e = np.empty((N_EDGES, 2), dtype=np.int64)
    e[:600] = rng.integers(0, n, (600, 2))
    e[0], e[1], e[2], e[100], e[200] = (n - 1, 0), (0, n - 1), (n - 1, n - 1), (n - 1, 5), (7, n - 1)
    e[DUP[0]] = e[DUP[1]]
    e[REV[0]] = e[REV[1]][:, ::-1]
    e[SELF] = rng.integers(0, n, 100)[:, None]
    e[NEG[0]] = e[NEG[1]] - n
    return e


EDGES = edge_list()

_HOST = {}


def host_matrix(d, which=0):
    key = (d, which)
    if key not in _HOST:
        _HOST[key] = np.ascontiguousarray(hash_matrix(N_ROWS, d, seed=77 * d + 13 * which + 5))
    return _HOST[key]


_REF = {}


def references(d, two=False, edges=EDGES):
    """(ref32, truth, cond) for A = host_matrix(d), B = A or host_matrix(d, 1): the reference's own two expressions
    torch.mm(A, B.t())[e0, e1] in float32 (ref32), the same in float64 (truth), and cond = sum_k |a_uk b_vk|"""
    key = (d, two)
    if key not in _REF or edges is not EDGES:
        a = torch.from_numpy(host_matrix(d))
        b = torch.from_numpy(host_matrix(d, 1)) if two else a
        e = torch.from_numpy(np.asarray(edges))
        e0, e1 = e[:, 0], e[:, 1]
        out = (torch.mm(a, b.t())[e0, e1].numpy(), torch.mm(a.double(), b.double().t())[e0, e1].numpy(),
               torch.mm(a.double().abs(), b.double().abs().t())[e0, e1].numpy())
        if edges is not EDGES:
            return out
        _REF[key] = out
    return _REF[key]


def gradient_references(d, two, g, edges=EDGES):
    """{dtype: (dA, dB or None)} by CPU autograd of the reference expression under the upstream gradient g, in float32 and float64,
    and under "cond" the sums of the absolute contributions per element (the same autograd on |A|, |B|, |g| in float64)"""
    e = torch.from_numpy(np.asarray(edges))
    out = {}
    for name, dt, absolute in (("ref32", torch.float32, False), ("truth", torch.float64, False), ("cond", torch.float64, True)):
        a = torch.from_numpy(host_matrix(d)).to(dt)
        b = torch.from_numpy(host_matrix(d, 1)).to(dt) if two else None
        gg = torch.from_numpy(g).to(dt)
        if absolute:
            a, b, gg = a.abs(), (None if b is None else b.abs()), gg.abs()
        a.requires_grad_(True)
        if b is not None:
            b.requires_grad_(True)
        sim = torch.mm(a, (a if b is None else b).t())
        (sim[e[:, 0], e[:, 1]].reshape(-1) * gg).sum().backward()
        out[name] = (a.grad.numpy(), None if b is None else b.grad.numpy())
    return out

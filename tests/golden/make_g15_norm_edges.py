#!/usr/bin/env python3
"""Generate tests/golden/g15_norm_edges.npz by IMPORTING THE REFERENCE ITSELF (as make_goldens.py does for g1 / g2).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g15_norm_edges.py

Needs /root/reference; nothing of the reference travels: the fixture holds inputs and recorded outputs only.

G15: the normalisation of ZERO, CANCELLING and NEGATIVE weights.  Two graphs of 48 nodes, the directed `edge48` and its
symmetrisation `edge48s`, stored here as (indptr, indices, data) because their stored zeros must survive (graphs.npz is loaded
through nothing that would drop them either, but these two are nobody else's business).  Each holds

  node 0    a_00 = -1 (cancels against the +1 of A + I) plus ordinary edges
  node 47   its only entry is a_ii = -1: its row of A + I is empty, its degree 0
  (5, 9)    a stored 0.0, in row 5 only: edge48s is symmetric in value, not in stored pattern
  (7, 12)   the duplicates +1.5, -1.5, summed to a stored 0
  node 14   a stored 0.0 on the diagonal
  node 20   degree exactly 0 through an off-diagonal -1, with in- and out-edges to ordinary nodes
  30, 31    two zero-degree nodes adjacent to each other
  node 35   degree -2; its neighbours in both directions (36, 37, 38, 39) all have positive degree
  node 40   isolated
  node 41   its only entry is the stored 0.0 at (41, 42)
and ordinary weights in [0.25, 3] everywhere else.

Recorded, per graph: for every variant of the suite's G1_VARIANTS (and PPR alpha = 1) the reference's `_construct_adj` result with ITS OWN indptr /
indices (scipy drops exact zeros at every stage, so the pattern depends on r and alpha) and fp64 data; and GraphOp.propagate
(K = 2, d = 5; Laplacian r = 0.5 and PPR (0.5, 0.15)) through the reference's own ctypes path, once on a finite hash_matrix x and
once with inf in the feature rows of nodes 31 and 41 -- rows that other rows reach only through a zero degree factor (31) or a
zero-weight edge (41).  The generator asserts where NaN appears (the negative degree at fractional r, nowhere else) and which
output rows are not finite, so that a scipy that behaves differently stops it instead of silently changing the truth."""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference"
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import scipy.sparse as sp

from inputs import hash_matrix  # noqa: E402

from sgl.operators.graph_op import LaplacianGraphOp, PprGraphOp  # noqa: E402

N = 48
VARIANTS = [("lap", r, None) for r in (0.0, 0.3, 0.5, 1.0)] + \
           [("ppr", 0.5, a) for a in (0.1, 0.15, 0.2, 0.3)] + [("ppr", 0.3, 0.15)]        # == the suite's G1_VARIANTS
VARIANTS += [("ppr", 0.5, 1.0)]                 # (1 - alpha) = 0: every finite entry of A_hat is dropped, alpha I and the NaNs stay
PROP = [("lap", 0.5, None), ("ppr", 0.5, 0.15)]
K, D = 2, 5
INF_ROWS = (31, 41)
ZERO_DEG = (20, 30, 31, 47)
NEG_DEG = 35
SPECIAL = (20, 30, 31, 35, 40, 41, 47)          # rows / columns the random ordinary edges stay away from

# (i, j, w, where): "out" = i -> j, "in" = j -> i, "both" = either direction in edge48; edge48s always holds both sides
PLANTED = [
    (0, 1, 1.0, "both"), (0, 2, 0.5, "out"),
    (20, 21, -1.0, "out"), (20, 22, 2.0, "out"), (20, 23, -2.0, "out"), (20, 24, 0.5, "in"), (20, 25, -0.5, "in"),
    (21, 22, 2.5, "both"), (22, 23, 2.5, "both"), (21, 23, 2.5, "both"), (24, 25, 2.0, "both"),
    (30, 31, -1.0, "both"), (30, 28, 0.75, "in"), (30, 29, -0.75, "in"), (28, 29, 2.0, "both"),
    (35, 36, -1.5, "out"), (35, 37, -1.5, "out"), (35, 38, 1.0, "in"), (35, 39, -1.0, "in"),
    (36, 37, 3.0, "both"), (38, 39, 3.0, "both"),
]
DIAGONAL = [(0, -1.0), (47, -1.0), (14, 0.0), (3, 1.25)]
ONE_SIDED_ZEROS = [(5, 9), (41, 42)]              # stored 0.0 in the row of the first node only, in both graphs
CANCELLING = (7, 12, 1.5)                         # +w and -w at the same place


def canonical(rows, cols, vals):
    """sorted CSR with duplicates summed in fp32 and every stored zero KEPT (numpy only: nothing here eliminates zeros)"""
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float32)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    new = np.ones(len(rows), dtype=bool)
    new[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    grp = np.cumsum(new) - 1
    data = np.zeros(grp[-1] + 1, dtype=np.float32)
    np.add.at(data, grp, vals)
    indptr = np.zeros(N + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[new], minlength=N), out=indptr[1:])
    return indptr, cols[new].astype(np.int32), data


def build(symmetric):
    rng = np.random.default_rng(15)                # the same draws for both graphs
    pool = np.array([i for i in range(N - 1) if i not in SPECIAL])
    taken = {(5, 9), (7, 12)} | {(min(i, j), max(i, j)) for i, j, _, _ in PLANTED}
    rows, cols, vals = [], [], []

    def add(i, j, w):
        rows.append(i); cols.append(j); vals.append(w)

    for _ in range(120):
        i, j = (int(v) for v in rng.choice(pool, 2, replace=False))
        w, w2 = (float(v) for v in rng.uniform(0.25, 3.0, 2).astype(np.float32))
        way = rng.random()
        if (min(i, j), max(i, j)) in taken:
            continue
        taken.add((min(i, j), max(i, j)))
        if symmetric:
            add(i, j, w); add(j, i, w)
        else:
            add(i, j, w)
            if way < 0.3:
                add(j, i, w2)
    for i, j, w, where in PLANTED:
        if symmetric or where in ("out", "both"):
            add(i, j, w)
        if symmetric or where in ("in", "both"):
            add(j, i, w)
    for i, w in DIAGONAL:
        add(i, i, w)
    for i, j in ONE_SIDED_ZEROS:
        add(i, j, 0.0)
    i, j, w = CANCELLING
    add(i, j, w); add(i, j, -w)
    if symmetric:
        add(j, i, w); add(j, i, -w)
    return canonical(rows, cols, vals)


def check_graph(name, indptr, indices, data):
    """the properties the fixture exists for, on the stored arrays (dense fp64 arithmetic is exact for these weights' sums)"""
    a = np.zeros((N, N))
    stored = np.zeros((N, N), dtype=bool)
    r = np.repeat(np.arange(N), np.diff(indptr))
    a[r, indices] = data
    stored[r, indices] = True
    deg = (a + np.eye(N)).sum(1)
    assert a[0, 0] == -1 and np.count_nonzero(a[0]) > 2 and deg[0] > 0
    assert stored[47].sum() == 1 and stored[:, 47].sum() == 1 and a[47, 47] == -1
    assert stored[5, 9] and a[5, 9] == 0 and not stored[9, 5]
    assert stored[41, 42] and stored[41].sum() == 1 and stored[:, 41].sum() == 0 and not stored[42, 41]
    assert stored[7, 12] and a[7, 12] == 0
    assert stored[14, 14] and a[14, 14] == 0
    assert not stored[40].any() and not stored[:, 40].any()
    assert sorted(np.nonzero(deg == 0)[0]) == list(ZERO_DEG), np.nonzero(deg == 0)
    assert list(np.nonzero(deg < 0)[0]) == [NEG_DEG] and deg[NEG_DEG] == -2
    nb = set(np.nonzero(a[NEG_DEG])[0]) | set(np.nonzero(a[:, NEG_DEG])[0])
    assert nb == {36, 37, 38, 39}
    assert all(deg[j] > 0 for j in nb)
    assert a[20, 21] == -1 and np.count_nonzero(a[:, 20]) >= 2 and a[30, 31] == -1 and a[31, 30] == -1
    if name == "edge48s":
        assert np.array_equal(a, a.T) and not np.array_equal(stored, stored.T)
    else:
        assert not np.array_equal(a, a.T)
    ordinary = data[(data != 0) & (np.abs(data) != 1) & (data > 0)]
    assert ordinary.min() >= 0.25 and ordinary.max() <= 3.0
    return a, deg


def main():
    out = {}
    x_fin = hash_matrix(N, D, seed=15)
    x_inf = x_fin.copy()
    x_inf[list(INF_ROWS)] = np.inf
    for name, symmetric in (("edge48", False), ("edge48s", True)):
        indptr, indices, data = build(symmetric)
        a, deg = check_graph(name, indptr, indices, data)
        out[name + "|indptr"], out[name + "|indices"], out[name + "|data"] = indptr, indices, data
        g = sp.csr_matrix((data, indices, indptr), shape=(N, N))
        assert g.nnz == len(data) and (g.data == 0).sum() >= 4           # the stored zeros are still there
        ap = a + np.eye(N)
        for kind, r, alpha in VARIANTS:
            op = LaplacianGraphOp(1, r=r) if kind == "lap" else PprGraphOp(1, r=r, alpha=alpha)
            adj = op._construct_adj(g)
            assert sp.isspmatrix_csr(adj) and adj.dtype == np.float64
            adj.sort_indices()
            key = f"{name}|{kind}|{r}" + ("" if alpha is None else f"|{alpha}")
            out[key + "|indptr"] = adj.indptr.astype(np.int32)
            out[key + "|indices"] = adj.indices.astype(np.int32)
            out[key + "|data"] = adj.data.astype(np.float64)
            assert not (adj.data == 0).any(), key                         # scipy stores no exact zero ...
            rows = np.repeat(np.arange(N), np.diff(adj.indptr))
            nan = np.isnan(adj.data)
            got = set(zip(rows[nan].tolist(), adj.indices[nan].tolist()))
            # ... and NaN exactly where the negative degree meets a fractional power: A_hat[j, i] = A'[i, j] L[j] R[i]
            want = {(j, i) for i in range(N) for j in range(N) if ap[i, j] != 0 and NEG_DEG in (i, j)} if r in (0.3, 0.5) else set()
            assert got == want and not np.isinf(adj.data).any(), (key, got ^ want)
            dense = adj.toarray()
            for z in ZERO_DEG:                                            # a zero degree: nothing stored but the PPR diagonal
                nz = set(np.nonzero(dense[z])[0]) | set(np.nonzero(dense[:, z])[0])
                if r in (0.3, 0.5):                                       # (r = 0 / 1: one factor is deg^0 = 1, half survives)
                    assert nz == (set() if alpha is None else {z}), (key, z, nz)
            if alpha is not None:
                assert dense[0, 0] == alpha and dense[47, 47] == alpha, key     # the cancelled diagonals hold alpha alone
            else:
                assert dense[0, 0] == 0 and adj.indptr[48] == adj.indptr[47], key
        for kind, r, alpha in PROP:
            for xname, x in (("fin", x_fin), ("inf", x_inf)):
                op = LaplacianGraphOp(K, r=r) if kind == "lap" else PprGraphOp(K, r=r, alpha=alpha)
                feats = op.propagate(g, x.copy())
                assert len(feats) == K + 1 and np.array_equal(feats[0].numpy(), x, equal_nan=True)
                key = f"{name}|{kind}|{r}" + ("" if alpha is None else f"|{alpha}") + f"|{xname}"
                for h in range(1, K + 1):
                    y = feats[h].numpy().copy()
                    assert y.dtype == np.float32
                    out[f"{key}|h{h}"] = y
                    bad = set(np.nonzero(~np.isfinite(y).all(1))[0].tolist())
                    if xname == "fin":
                        out_nb = set(np.nonzero(ap[NEG_DEG])[0].tolist()) | {NEG_DEG}
                        assert bad >= out_nb if h == 1 else bad > out_nb, (key, h, bad)
                    else:
                        fin = set(np.nonzero(~np.isfinite(out[f"{key[:-4]}|fin|h{h}"]).all(1))[0].tolist())
                        # the inf rows poison nobody else; 31 itself only through the PPR diagonal, 41 through its own diagonal
                        assert bad - fin == ({41} if alpha is None else {31, 41}), (key, h, bad - fin)
    out["x_fin"], out["x_inf"] = x_fin, x_inf
    np.savez_compressed(os.path.join(HERE, "g15_norm_edges.npz"), **out)


if __name__ == "__main__":
    main()

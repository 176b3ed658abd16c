#!/usr/bin/env python3
"""Generate tests/golden/g20_transforms.npz by IMPORTING THE REFERENCE ITSELF (as make_g17_edge_split.py does).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g20_transforms.py <path of the reference checkout>

Needs the reference checkout (the directory that holds its `sgl` package); nothing of the reference travels: the fixture holds the
inputs made here and recorded outputs only.

G20: the graph transforms of sgl/data/transforms.py on the graphs sym64, pl256 and dir40 of graphs.npz and on symdiag48, a symmetric
graph with symmetric weights and a non-zero diagonal that is made (and stored) here.  For each graph an Edge is built from the COO of
the canonical CSR, so the reference's edge order IS the CSR entry order, and with a fixed edge mask and a fixed node mask (stored)
the `sparse_matrix` of these results is recorded as canonical CSR arrays:

    drop      drop_edges(edge, n, edge_mask)
    drop_und  drop_edges(edge, n, edge_mask, force_undirected=True)
    noself    remove_self_loops(edge, n)
    sub       the two lines get_subgraph delegates to with keep_ids=False: edge_mask = node_mask[row] & node_mask[col];
              drop_edges(edge, n_remain, edge_mask, node_id_dict={old: new})
    sub_keep  the same with keep_ids=True: drop_edges(edge, n, edge_mask)

get_subgraph itself is not called because it cannot run as shipped: it turns a BoolTensor mask into a numpy array and then calls
`node_mask.dim()` on it, which raises AttributeError (a list is turned into a numpy array too).  The two delegated lines run when
called by hand, and they are what the function would compute.

drop_edges(force_undirected=True) writes into the mask it is given: every call below gets its own clone."""
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np
import scipy.sparse as sp
import torch

GRAPHS = ("sym64", "pl256", "dir40", "symdiag48")
SEED = 20


def canonical(a):
    a = sp.csr_matrix(a)
    a.sum_duplicates()
    a.sort_indices()
    return a


def graph(name):
    g = np.load(os.path.join(HERE, "graphs.npz"))
    indptr, indices, data = g[name + "|indptr"], g[name + "|indices"], g[name + "|data"]
    n = len(indptr) - 1
    return canonical(sp.csr_matrix((data.astype(np.float32), indices, indptr), shape=(n, n)))


def symdiag48():
    """48 nodes, about 6 neighbours each, symmetric float32 weights, 30 of the 48 diagonal entries stored"""
    rng = np.random.RandomState(SEED)
    n = 48
    upper = sp.triu(sp.random(n, n, density=0.13, random_state=rng, format="csr", dtype=np.float32), k=1)
    upper.data = (0.25 + rng.rand(upper.nnz)).astype(np.float32)
    diag = np.where(rng.rand(n) < 0.6, 0.125 + rng.rand(n), 0.0).astype(np.float32)
    a = canonical(upper + upper.T + sp.diags(diag, format="csr", dtype=np.float32))
    a.eliminate_zeros()
    assert (a != a.T).nnz == 0 and (a.diagonal() != 0).sum() > 10
    return canonical(a.astype(np.float32))


def reference_transforms():
    if "sgl.data" not in sys.modules:                  # the package's __init__ would do, but this keeps the import to two files
        pkg = types.ModuleType("sgl.data")
        pkg.__path__ = [REF + "/sgl/data"]
        sys.modules["sgl.data"] = pkg
    import sgl.data.base_data as base_data
    import sgl.data.transforms as transforms
    return base_data, transforms


def put(out, key, m):
    m = canonical(m)
    out[key + "|indptr"] = m.indptr.astype(np.int64)
    out[key + "|indices"] = m.indices.astype(np.int32)
    out[key + "|data"] = m.data.astype(np.float32)
    out[key + "|shape"] = np.array(m.shape, dtype=np.int64)


def main():
    base_data, tr = reference_transforms()
    out = {"graphs": np.array(GRAPHS)}
    put(out, "symdiag48", symdiag48())
    rng = np.random.RandomState(SEED + 1)
    for name in GRAPHS:
        a = symdiag48() if name == "symdiag48" else graph(name)
        n = a.shape[0]
        coo = a.tocoo()                                 # of a canonical CSR: row by row, columns ascending
        assert np.array_equal(coo.col, a.indices) and np.all(np.diff(coo.row) >= 0)

        def edge():
            return base_data.Edge(torch.from_numpy(coo.row.astype(np.int64)), torch.from_numpy(coo.col.astype(np.int64)),
                                  torch.from_numpy(coo.data.astype(np.float32)), "e", n)

        edge_mask = rng.rand(a.nnz) < 0.6
        node_mask = rng.rand(n) < 0.55
        out[f"{name}|edge_mask"] = edge_mask
        out[f"{name}|node_mask"] = node_mask
        put(out, f"{name}|drop", tr.drop_edges(edge(), n, torch.from_numpy(edge_mask.copy())).sparse_matrix)
        put(out, f"{name}|drop_und", tr.drop_edges(edge(), n, torch.from_numpy(edge_mask.copy()), force_undirected=True).sparse_matrix)
        put(out, f"{name}|noself", tr.remove_self_loops(edge(), n).sparse_matrix)
        nm = torch.from_numpy(node_mask.copy())
        row, col = edge().edge_index
        sub_mask = nm[row] & nm[col]
        remain = np.arange(n)[node_mask]
        put(out, f"{name}|sub", tr.drop_edges(edge(), len(remain), sub_mask.clone(), node_id_dict={int(old): new for new, old in enumerate(remain)}).sparse_matrix)
        put(out, f"{name}|sub_keep", tr.drop_edges(edge(), n, sub_mask.clone()).sparse_matrix)
        print(name, n, a.nnz, {k: int(out[f"{name}|{k}|indices"].size) for k in ("drop", "drop_und", "noself", "sub", "sub_keep")})
    np.savez_compressed(os.path.join(HERE, "g20_transforms.npz"), **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/g24_meta_path.npz by IMPORTING THE REFERENCE ITSELF (as make_g23_hetero.py does).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g24_meta_path.py <path of the reference checkout>

G24: HeteroNodeDataset.sample_by_meta_path of the reference on a toy graph -- 3 node types in the order author 6, paper 9, field 4,
d = 3, three relations stored in both directions (author / paper, paper / field, author / field; no paper__to__paper), edge lists
with repeats.  The LAST node of every type occurs in every edge list: the reference infers each factor's shape from the
largest id present, and its product exists only when those agree.  Recorded: the constructor arguments (graph|...) and, for every
path of PATHS with and without `undirected`, the canonical CSR, the stacked features and node_id (sample|<k>|...).

The reference is imported by make_g23_hetero.py, under its shims (a torch proxy whose from_numpy passes tensors through; the stub
recipe of SURVEY.md Appendix B).  Nothing of the reference travels: the fixture holds the inputs made here and recorded outputs only."""
import os

import numpy as np

from make_g23_hetero import HeteroGraph, ref_dataset  # noqa: E402  (the reference, imported under that script's shims; same argument)

HERE = os.path.dirname(os.path.abspath(__file__))
NODE_TYPES = ["author", "paper", "field"]
NUM = {"author": 6, "paper": 9, "field": 4}
N_EDGES = {"author__to__paper": 14, "paper__to__field": 11, "author__to__field": 5}
EDGE_TYPES = ["author__to__paper", "paper__to__author", "paper__to__field", "field__to__paper", "author__to__field", "field__to__author"]
# the first type before, after and equal to the last one in NODE_TYPES; a chain of three factors
PATHS = ["author__to__paper__to__field", "field__to__paper__to__author", "paper__to__author__to__paper", "paper__to__field__to__paper",
         "author__to__paper__to__field__to__paper"]
D = 3


def main():
    rng = np.random.default_rng(24)
    offsets = {t: sum(NUM[u] for u in NODE_TYPES[:i]) for i, t in enumerate(NODE_TYPES)}
    rows, cols = {}, {}
    for e, n_edges in N_EDGES.items():
        src, _, dst = e.split("__")
        r, c = rng.integers(0, NUM[src], n_edges), rng.integers(0, NUM[dst], n_edges)
        r[0], c[1] = NUM[src] - 1, NUM[dst] - 1                      # the last node of both types
        r[-2:], c[-2:] = r[:2], c[:2]                                # repeats
        rows[e], cols[e] = (r + offsets[src]).astype(np.int64), (c + offsets[dst]).astype(np.int64)
        back = dst + "__to__" + src
        rows[back], cols[back] = cols[e].copy(), rows[e].copy()
    x = {t: rng.standard_normal((NUM[t], D)).astype(np.float32) for t in NODE_TYPES}
    graph = HeteroGraph(dict(rows), dict(cols), {e: np.ones(len(rows[e]), np.float32) for e in EDGE_TYPES}, dict(NUM), list(NODE_TYPES),
                        list(EDGE_TYPES), None, dict(x), {})
    ds = object.__new__(ref_dataset.HeteroNodeDataset)               # (its __init__ downloads and processes files)
    ds._name, ds._data = "g24", graph
    out = {"graph|node_types": np.array(NODE_TYPES), "graph|num": np.array([NUM[t] for t in NODE_TYPES]), "graph|edge_types": np.array(EDGE_TYPES)}
    for e in EDGE_TYPES:
        out[f"graph|row|{e}"], out[f"graph|col|{e}"] = rows[e], cols[e]
    for t in NODE_TYPES:
        out[f"graph|x|{t}"] = x[t]
    k = 0
    for path in PATHS:
        for undirected in (True, False):
            adj, feature, node_id = ds.sample_by_meta_path(path, undirected)
            adj = adj.tocsr().copy()
            adj.sum_duplicates()
            adj.sort_indices()
            assert np.all(adj.data == 1.0) and feature.dtype == np.float32
            out[f"sample|{k}|path"], out[f"sample|{k}|undirected"] = np.array(path), np.array(undirected)
            out[f"sample|{k}|rowptr"], out[f"sample|{k}|col"] = adj.indptr.astype(np.int64), adj.indices.astype(np.int32)
            out[f"sample|{k}|x"], out[f"sample|{k}|node_id"] = feature, node_id.numpy().astype(np.int64)
            k += 1
    path = os.path.join(HERE, "g24_meta_path.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays,", k, "samples")


if __name__ == "__main__":
    main()

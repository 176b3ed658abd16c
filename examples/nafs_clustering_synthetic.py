#!/usr/bin/env python3
"""The NAFS node-clustering task (NodeClusteringNAFS: hops = range(K), several r values, KMeans and three scores per hop count;
sgl/tasks/node_clustering.py:121-258) end to end on the MI355X, on a planted-partition graph.

`nafs_node_clustering` runs ONE propagation per r for all hop counts (nafs_ensemble_sweep) and clusters each hop count's features
where they lie: k-means with the assignment kernel (sgl_kmeans_assign_f32) and the membership-matrix SpMM as the centre update, then
acc / nmi / adjscore from one contingency table.  Nothing but the graph and the features is uploaded, and nothing but three floats
per hop count comes back.

    python examples/nafs_clustering_synthetic.py [--nodes 20000] [--hops 8] [--classes 5] [--method mean]
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgl_amd.tricks import nafs_node_clustering  # noqa: E402


def planted_partition(n, classes, deg, p_in, d, seed):
    """n nodes in `classes` blocks, about `deg` neighbours each, a share p_in of them in the node's own block; features: a weak block
    indicator under unit noise"""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, classes, n)
    order = np.argsort(y, kind="stable")
    start = np.searchsorted(y[order], np.arange(classes + 1))
    a = np.repeat(np.arange(n), deg)
    b = rng.integers(0, n, a.size)
    inside = rng.random(a.size) < p_in
    ya = y[a[inside]]
    b[inside] = order[start[ya] + (rng.random(ya.size) * (start[ya + 1] - start[ya])).astype(np.int64)]
    adj = sp.coo_matrix((np.ones(a.size, np.float32), (a, b)), shape=(n, n)).tocsr()
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()
    x = rng.standard_normal((n, d)).astype(np.float32) + np.eye(classes, d, dtype=np.float32)[y]
    return adj, x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20_000)
    ap.add_argument("--hops", type=int, default=8)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--method", default="mean", choices=("mean", "max", "concat", "simple"))
    ap.add_argument("--n-init", type=int, default=5)
    a = ap.parse_args()
    adj, x, y = planted_partition(a.nodes, a.classes, 10, 0.8, 32, seed=0)
    t0 = time.time()
    res = nafs_node_clustering(adj, x, y, a.hops, r_list=(0.5, 0.3, 0), method=a.method, n_init=a.n_init, seed=42)
    took = time.time() - t0
    print(f"{a.nodes} nodes, {adj.nnz} edges, {a.classes} blocks, method {a.method}, n_init {a.n_init}: {took:.2f} s")
    print("hops    acc     nmi     adjscore")
    for hop in range(a.hops):
        acc, nmi, adjscore = res.metrics[hop]
        print(f"{hop:4d}  {acc:.4f}  {nmi:.4f}  {adjscore:.4f}")
    print(f"best: acc {res.acc:.4f} at {res.best_hop_acc} hops, nmi {res.nmi:.4f} at {res.best_hop_nmi}, "
          f"adjscore {res.adjscore:.4f} at {res.best_hop_adjscore}")


if __name__ == "__main__":
    main()

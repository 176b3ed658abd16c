#!/usr/bin/env python3
"""Generate tests/golden/g16_node_clustering.npz by IMPORTING THE REFERENCE ITSELF (as make_g14_link_prediction.py does).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g16_node_clustering.py

Needs /root/reference, sklearn and scipy; nothing of the reference travels: the fixture holds inputs and recorded outputs only.
`munkres` is not installed where this runs, and the reference's clusteringAcc USES what Munkres().compute returns, so a MagicMock
would not do: a stand-in Munkres is installed whose compute() wraps scipy.optimize.linear_sum_assignment (the matched count of an
optimal one-to-one matching is unique even where the matching is not, so the accuracy is the one Munkres gives).

G16 holds three things.
(a) Fixed-init Lloyd parity: four blob sets (n, d, k, spread of the centres), unit noise, c0 = k seeded rows of x -- inputs that
    tests/kmeans_common.blob_set regenerates bit for bit, so only the outputs are stored; sklearn's
    KMeans(init=c0, n_init=1, algorithm="lloyd") labels, centres (float32), inertia and n_iter_, and the same loop in numpy float64
    (truth).  Asserted here: every set ends by unchanged labels, sklearn's iteration count and labels equal the float64 loop's,
    and no row of the final assignment is near a tie.  If an assertion fails the SEED (kmeans_common.BLOB_SEEDS) changes, not the assertion.
(b) Three (labels_true, labels_pred) sets -- a permuted perfect match, a noisy match, fewer predicted clusters than classes -- with the
    reference's (acc, nmi, adjscore); for the third the reference raises (clusteringAcc returns a bare 0 that its caller cannot
    unpack), so nmi and adjscore come from sklearn directly and acc is recorded as 0.
(c) NodeClusteringNAFS itself on a planted-partition graph (stored here) of 288 nodes in 4 blocks, features a noisy block indicator
    (d = 12; one node in ten shows another block's, which propagation corrects), r_list [0.5, 0.3, 0], hops {0, 1, 3, 6}, all four methods: the per-hop scores and the six best values.  Asserted for
    every (method, hop): sklearn reaches the same partition at five random_states -- only then is a comparison of scores meaningful."""
import importlib
import os
import sys
import types
from unittest.mock import MagicMock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference"
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np
import scipy.sparse as sp
import torch
from scipy.optimize import linear_sum_assignment
from sklearn import metrics as skm
from sklearn.cluster import KMeans

from kmeans_common import BLOBS, blob_set  # noqa: E402

METHODS = ("mean", "max", "concat", "simple")
HOPS = (0, 1, 3, 6)
R_LIST = [0.5, 0.3, 0]


class Munkres:
    """stand-in for munkres.Munkres: compute(cost) -> [(row, column), ...] of a minimum-cost one-to-one matching"""

    def compute(self, cost):
        rows, cols = linear_sum_assignment(np.asarray(cost))
        return list(zip(rows.tolist(), cols.tolist()))


def reference_task_module():
    for m in ["matplotlib", "matplotlib.pyplot"]:
        try:
            importlib.import_module(m)
        except ImportError:
            sys.modules[m] = MagicMock()
    try:
        importlib.import_module("munkres")
    except ImportError:
        stand_in = types.ModuleType("munkres")
        stand_in.Munkres = Munkres
        sys.modules["munkres"] = stand_in
    if "sgl.tasks" not in sys.modules:
        pkg = types.ModuleType("sgl.tasks")
        pkg.__path__ = [REF + "/sgl/tasks"]
        sys.modules["sgl.tasks"] = pkg
    import sgl.tasks.node_clustering as nc
    return nc


def dist64(x, c):
    return ((x[:, None, :].astype(np.float64) - c[None, :, :].astype(np.float64)) ** 2).sum(-1)


def lloyd64(x, c0, tol=1e-4, max_iter=300):
    """sklearn's _kmeans_single_lloyd in float64: (labels, centres, inertia, n_iter, ended by unchanged labels)"""
    x64 = x.astype(np.float64)
    tol_abs = tol * np.mean(np.var(x64, axis=0))
    c = c0.astype(np.float64)
    old = None
    strict = False
    for it in range(max_iter):
        labels = dist64(x, c).argmin(1)
        new = np.stack([x64[labels == j].mean(0) for j in range(len(c))])
        shift = ((new - c) ** 2).sum()
        c = new
        if old is not None and np.array_equal(labels, old):
            strict = True
            break
        if shift <= tol_abs:
            break
        old = labels
    if not strict:
        labels = dist64(x, c).argmin(1)
    return labels, c, float(dist64(x, c)[np.arange(len(x)), labels].sum()), it + 1, strict


def near_tie_rows(x, c):
    d = x.shape[1]
    two = np.sort(dist64(x, c), axis=1)[:, :2]
    return int(((two[:, 1] - two[:, 0]) <= (d + 3) * 2.0 ** -22 * two[:, 1]).sum())


def planted_partition(n, blocks, p_in, p_out, seed):
    rng = np.random.default_rng(seed)
    block = np.repeat(np.arange(blocks), n // blocks)
    prob = np.where(block[:, None] == block[None, :], p_in, p_out)
    upper = np.triu(rng.random((n, n)) < prob, 1)
    a = sp.csr_matrix((upper | upper.T).astype(np.float32))
    return a, block.astype(np.int64)


def main():
    nc = reference_task_module()
    out = {}

    # (a) fixed-init Lloyd parity
    for n, d, k, spread in BLOBS:
        x, y, c0 = blob_set(n, d, k, spread)                # regenerated by the tests (tests/kmeans_common.py), not stored
        km = KMeans(n_clusters=k, init=c0, n_init=1, algorithm="lloyd").fit(x)
        labels, centres, inertia, n_iter, strict = lloyd64(x, c0)
        key = f"lloyd|{n}x{d}x{k}"
        assert strict, (key, "did not end by unchanged labels")
        assert km.n_iter_ == n_iter, (key, km.n_iter_, n_iter)
        assert np.array_equal(km.labels_, labels), key
        assert near_tie_rows(x, centres) == 0, key
        print(key, "iterations", n_iter, "inertia", inertia, km.inertia_)
        out[key + "|labels"] = km.labels_.astype(np.int64)
        out[key + "|centres"] = km.cluster_centers_.astype(np.float32)
        out[key + "|inertia"] = np.array([km.inertia_], dtype=np.float64)
        out[key + "|n_iter"] = np.array([km.n_iter_], dtype=np.int64)
        out[key + "|truth_centres"] = centres
        out[key + "|truth_inertia"] = np.array([inertia], dtype=np.float64)
        if (n, d, k) in ((600, 16, 3), (1500, 100, 7)):
            for state in range(5):                   # a single optimum: the generating partition at every random_state
                got = KMeans(n_clusters=k, n_init=5, random_state=state).fit_predict(x)
                assert skm.adjusted_rand_score(y, got) == 1.0, (key, state)

    # (b) metric sets
    rng = np.random.default_rng(1616)
    true = rng.integers(0, 6, 700)
    perm = rng.permutation(6)
    noisy = np.where(rng.random(700) < 0.25, rng.integers(0, 6, 700), perm[true])
    sets = {"perfect": (true, perm[true]), "noisy": (true, noisy), "fewer": (true, np.minimum(perm[true], 3))}
    for name, (t, p) in sets.items():
        cm = nc.clustering_metrics(t, p)
        try:
            acc, nmi, adjscore = cm.evaluationClusterModelFromLabel()
            raised = 0
        except TypeError:                            # clusteringAcc returned a bare 0
            acc, nmi, adjscore = 0.0, skm.normalized_mutual_info_score(t, p), skm.adjusted_rand_score(t, p)
            raised = 1
        assert raised == (name == "fewer"), name
        print("metrics", name, acc, nmi, adjscore)
        out[f"metrics|{name}|true"], out[f"metrics|{name}|pred"] = t.astype(np.int64), p.astype(np.int64)
        out[f"metrics|{name}|scores"] = np.array([acc, nmi, adjscore], dtype=np.float64)
        out[f"metrics|{name}|reference_raised"] = np.array([raised], dtype=np.int64)

    # (c) the task itself
    adj, block = planted_partition(288, 4, 0.15, 0.005, seed=16)
    rng = np.random.default_rng(17)
    shown = np.where(rng.random(288) < 0.10, rng.integers(0, 4, 288), block)     # one node in ten shows another block's indicator
    x = (2.0 * np.eye(4, 12)[shown] + 0.3 * rng.standard_normal((288, 12))).astype(np.float32)
    y = block
    assert len(np.unique(y)) == 4 and (shown != block).sum() > 10

    class DS:
        num_node = 288
        num_classes = 4
    DS.adj, DS.x, DS.y = adj, x, torch.from_numpy(y)

    class CheckedKMeans(KMeans):
        """the task's KMeans, plus the assertion that makes its scores comparable: one partition at five random_states"""

        def fit_predict(self, feats, *a, **kw):
            got = super().fit_predict(feats, *a, **kw)
            for state in range(5):
                other = KMeans(n_clusters=self.n_clusters, n_init=5, random_state=state).fit_predict(feats)
                assert skm.adjusted_rand_score(got, other) == 1.0, ("partition depends on the seeding", state, feats.shape)
            return got

    nc.KMeans = CheckedKMeans
    coo = adj.tocoo()
    out["task|row"], out["task|col"] = coo.row.astype(np.int64), coo.col.astype(np.int64)
    out["task|x"], out["task|y"] = x, y
    out["task|hops"], out["task|r_list"] = np.array(HOPS), np.array(R_LIST, dtype=np.float64)
    for method in METHODS:
        task = object.__new__(nc.NodeClusteringNAFS)
        for name, value in (("dataset", DS), ("labels", DS.y), ("method", method), ("r_list", list(R_LIST)), ("hops", list(HOPS)),
                            ("seed", 42), ("n_clusters", 4), ("n_init", 20)):
            setattr(task, "_NodeClusteringNAFS__" + name, value)
        for hop in HOPS:
            out[f"task|{method}|hops{hop}"] = np.array(task._k_hop_cluster(hop), dtype=np.float64)
        best = task._execute()
        out[f"task|{method}|best"] = np.array(best, dtype=np.float64)
        print(method, [out[f"task|{method}|hops{h}"].round(4).tolist() for h in HOPS], best)
    path = os.path.join(HERE, "g16_node_clustering.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

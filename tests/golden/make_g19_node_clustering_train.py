#!/usr/bin/env python3
"""Generate tests/golden/g19_node_clustering_train.npz by IMPORTING THE REFERENCE ITSELF (as make_g16_node_clustering.py and
make_g18_gae_link_prediction.py do).

    PYTHONDONTWRITEBYTECODE=1 SGL_REFERENCE=<checkout of the reference> python tests/golden/make_g19_node_clustering_train.py

Needs the reference, sklearn and scipy; nothing of the reference travels: the fixture holds inputs and recorded outputs only.  As in
make_g16 a stand-in `munkres.Munkres` wraps scipy.optimize.linear_sum_assignment where munkres is not installed.

G19 holds two things.
(a) step|*  the reference's own cluster_loss (sgl/tasks/utils.py:101-113, Python loop included) and the .grad of a leaf output for
    fixed (Z, y_pred, centres), in float32 and in float64 (the same float32 inputs, widened): Z = the model of (b) at its saved state
    applied to x, centres = the member means of the planted partition with centre 0 replaced by an exact copy of a row (a zero
    distance), y_pred = the planted labels with one in eight redrawn.
(b) task|*  NodeClustering._execute (sgl/tasks/node_clustering.py:54-119) -- three epochs of the reference's clustering_train
    (sgl/tasks/utils.py:116-136) and its final clustering step -- on kmeans_common.blob_set(600, 16, 3, 3.0): a planted-partition graph
    whose blocks are the blobs, with self loops (stored here: tests/golden/graphs.npz has no planted graph), x = two hops of the symmetrically
    normalised graph applied to the blob features, an SGC-like model (one Linear layer, 16 -> 8, on x) from the saved state_dict,
    Adam(lr = 0.01), float32 and float64; the labels the scores are taken against are the planted ones with one in ten redrawn, so
    that the three scores are not trivially 1.  Recorded: per-epoch loss and scores, the final scores, the three bests, and per epoch
    the sum of the absolute contributions to the loss (float64 run).  The model subclass has a postprocess that accepts the task's
    single-argument call (BaseSGAPModel.postprocess(adj, output) does not: the reference raises at its final step).

The reference leaves KMeans unseeded, so parity is defined only where k-means is unique.  Asserted here, for five numpy seeds and both
dtypes: every epoch's y_pred is the planted partition up to renaming; every epoch's cluster_centers_ equal their members' means to
float32 rounding (strict Lloyd convergence, not a stop by tol); the per-epoch losses of the five seeds agree to within the
float32-vs-float64 gap (or 16 float32 roundings of the sum of the absolute contributions, the floor of oracle.truth_report).  If a blob
set does not meet this, a wider spread is chosen, not a looser assertion."""
import importlib
import os
import sys
import types
from unittest.mock import MagicMock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ["SGL_REFERENCE"]                  # a checkout of the reference project
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
from scipy.optimize import linear_sum_assignment
from sklearn import metrics as skm
from sklearn.cluster import KMeans

from kmeans_common import blob_set  # noqa: E402

BLOB = (600, 16, 3, 3.0)
HIDDEN, EPOCHS, LR, SEEDS = 8, 3, 0.01, (0, 1, 2, 3, 4)
FLOOR = 16 * 2.0 ** -24


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


def planted_graph(block, p_in, p_out, seed):
    rng = np.random.default_rng(seed)
    n = len(block)
    prob = np.where(block[:, None] == block[None, :], p_in, p_out)
    upper = np.triu(rng.random((n, n)) < prob, 1)
    return sp.csr_matrix((upper | upper.T).astype(np.float32))


def sgc_model(base, f_in, dtype):
    """one Linear layer on the pre-propagated features: BaseSGAPModel without graph operators; postprocess takes the task's call"""
    class SGCLike(base):
        def __init__(self):
            super().__init__(2, f_in, HIDDEN)
            self._base_model = nn.Linear(f_in, HIDDEN).to(dtype)

        def postprocess(self, output, *unused):
            return output
    return SGCLike()


def main():
    nc = reference_task_module()
    import sgl.tasks.utils as ut
    for m in ["torch_geometric", "torch_geometric.data", "torch_geometric.datasets", "torch_geometric.io", "torch_geometric.utils",
              "torch_sparse", "ogb", "ogb.nodeproppred", "gensim", "gensim.models", "openbox"]:
        sys.modules.setdefault(m, MagicMock())       # what the reference's dataset modules import and a model without operators never uses
    import sgl.dataset  # noqa: F401  (must come first: circular import)
    from sgl.models.base_model import BaseSGAPModel

    n, d, k, spread = BLOB
    feats, block, _ = blob_set(n, d, k, spread)
    g = (planted_graph(block, 0.10, 0.002, seed=19) + sp.identity(n, dtype=np.float32, format="csr")).tocsr()
    deg = np.asarray(g.sum(1)).reshape(-1)
    assert deg.min() > 0
    dinv = sp.diags(deg ** -0.5)
    norm = (dinv @ g @ dinv).tocsr()
    x = np.ascontiguousarray((norm @ (norm @ feats.astype(np.float64))).astype(np.float32))
    rng = np.random.default_rng(1919)
    y = np.where(rng.random(n) < 0.10, rng.integers(0, k, n), block).astype(np.int64)
    assert len(np.unique(y)) == k and (y != block).sum() > 10
    coo = g.tocoo()
    out = {"task|row": coo.row.astype(np.int32), "task|col": coo.col.astype(np.int32), "task|x": x, "task|y": y, "task|block": block,
           "task|epochs": np.array(EPOCHS), "task|lr": np.array(LR)}
    torch.manual_seed(19)
    state = {key: v.clone() for key, v in sgc_model(BaseSGAPModel, d, torch.float32).state_dict().items()}
    for key, v in state.items():
        out["task|state|" + key] = v.numpy().copy()

    # ---- (a) one loss and its gradient, the reference's literal expression
    z = (torch.from_numpy(x) @ state["_base_model.weight"].t() + state["_base_model.bias"]).numpy().copy()
    centres = np.stack([z[block == j].astype(np.float64).mean(0) for j in range(k)]).astype(np.float32)
    centres[0] = z[7]
    y_pred = np.where(rng.random(n) < 0.125, rng.integers(0, k, n), block).astype(np.int64)
    out["step|z"], out["step|centres"], out["step|labels"] = z, centres, y_pred
    for tag, dtype in (("", torch.float32), ("64", torch.float64)):
        leaf = torch.from_numpy(z).to(dtype).requires_grad_(True)
        loss = ut.cluster_loss(leaf, y_pred, torch.from_numpy(centres).to(dtype))
        loss.backward()
        assert bool(torch.isfinite(leaf.grad).all())
        out["step|loss" + tag] = np.array(float(loss.detach()), dtype=np.float64)
        out["step|grad" + tag] = leaf.grad.numpy().copy()
    print("step", out["step|loss"], out["step|loss64"], np.abs(out["step|grad"] - out["step|grad64"]).max())

    # ---- (b) the task, five numpy seeds, both dtypes
    class DS:
        adj = g
        num_node = n
        num_classes = k
    DS.y = torch.from_numpy(y)
    seen = {}                                        # what the task's KMeans saw in the current run

    class CheckedKMeans(KMeans):
        """the task's KMeans, plus the assertions that make its run comparable"""

        def fit_predict(self, f, *a, **kw):
            got = super().fit_predict(f, *a, **kw)
            assert skm.adjusted_rand_score(block, got) == 1.0, "y_pred is not the planted partition"
            means = np.stack([np.asarray(f, dtype=np.float64)[got == j].mean(0) for j in range(self.n_clusters)])
            gap = np.abs(self.cluster_centers_ - means).max()
            assert gap <= FLOOR * np.abs(means).max(), ("the centres are not their members' means", gap)
            seen.setdefault("fits", []).append((np.asarray(f, dtype=np.float64).copy(), got.copy(), self.cluster_centers_.astype(np.float32)))
            return got

    nc.KMeans = ut.KMeans = CheckedKMeans
    train = ut.clustering_train
    runs = {}
    for tag, dtype in (("", torch.float32), ("64", torch.float64)):
        for seed in SEEDS:
            np.random.seed(seed)
            model = sgc_model(BaseSGAPModel, d, dtype)
            model.load_state_dict({key: v.to(dtype) for key, v in state.items()})
            DS.x = torch.from_numpy(x).to(dtype)
            steps = []
            seen.clear()

            def recording(*a, **kw):
                r = train(*a, **kw)
                steps.append(r)
                return r

            nc.clustering_train = recording
            task = object.__new__(nc.NodeClustering)
            p = "_NodeClustering__"
            for name, value in (("dataset", DS), ("labels", DS.y), ("model", model), ("epochs", EPOCHS), ("loss_fn", ut.cluster_loss),
                                ("optimizer", torch.optim.Adam(model.parameters(), lr=LR, weight_decay=0.0)), ("device", torch.device("cpu")),
                                ("seed", 42), ("cluster_train_idx", torch.arange(0, n, dtype=torch.long)), ("n_clusters", k), ("n_init", 20)):
                setattr(task, p + name, value)
            best = task._execute()
            nc.clustering_train = train
            final = getattr(task, p + "model")
            fits = seen["fits"]
            assert len(steps) == EPOCHS and len(fits) == EPOCHS + 1
            cond = []
            for f, got, cen in fits[:EPOCHS]:        # sum of the absolute contributions to each epoch's loss
                dist = np.sqrt(((f[:, None, :] - cen[None].astype(np.float64)) ** 2).sum(-1))
                wgt = np.abs(2.0 * (got[:, None] == np.arange(k)[None]) - 1.0 / k)
                cond.append((wgt * dist).sum() / n)
            cm = nc.clustering_metrics(y, fits[-1][1])
            runs[(tag, seed)] = dict(loss=np.array([s[0] for s in steps]), scores=np.array([s[1:] for s in steps], dtype=np.float64),
                                     final=np.array(cm.evaluationClusterModelFromLabel(), dtype=np.float64), best=np.array(best, dtype=np.float64),
                                     cond=np.array(cond), state={key: v.detach().numpy().copy() for key, v in final.state_dict().items()})
    first32, first64 = runs[("", SEEDS[0])], runs[("64", SEEDS[0])]
    gap = np.abs(first32["loss"] - first64["loss"])
    allowed = np.maximum(gap, FLOOR * first64["cond"])
    for (tag, seed), r in runs.items():
        base = first32 if tag == "" else first64
        assert (np.abs(r["loss"] - base["loss"]) <= allowed).all(), (tag, seed, r["loss"], base["loss"], allowed)
        assert np.array_equal(r["scores"], base["scores"]) and np.array_equal(r["final"], base["final"]) and np.array_equal(r["best"], base["best"])
    assert np.array_equal(first32["scores"], first64["scores"]) and np.array_equal(first32["final"], first64["final"])
    for tag, r in (("", first32), ("64", first64)):
        out["task|loss" + tag] = r["loss"].astype(np.float64)
    out["task|loss_cond"] = first64["cond"]
    out["task|scores"], out["task|final"], out["task|best"] = first32["scores"], first32["final"], first32["best"]
    for key, v in first32["state"].items():
        out["task|final_state|" + key] = v
    path = os.path.join(HERE, "g19_node_clustering_train.npz")
    np.savez_compressed(path, **out)
    print({key: (v.shape, v.dtype) for key, v in out.items()})
    print(out["task|loss"], out["task|loss64"], out["task|loss_cond"], out["task|scores"], out["task|final"], out["task|best"])
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

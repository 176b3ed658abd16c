#!/usr/bin/env python3
"""Generate tests/golden/g14_link_prediction.npz by IMPORTING THE REFERENCE ITSELF (as make_goldens.py does for g11).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g14_link_prediction.py

Needs /root/reference and sklearn (what the reference's edge_predict_score calls); nothing of the reference travels: the fixture
holds inputs and recorded outputs only.

G14: LinkPredictionNAFS._k_hop_link_prediction (sgl/tasks/link_prediction.py:233-284) on graph pl256, x = hash_positive(256, 12,
seed=41), r_list [0.5, 0.3, 0], 200 positive edges taken from the graph and 200 seeded random pairs as negatives, for every
ensemble method x hops in {0, 1, 3, 6}: the float32 logits sim[e0, e1] of the reference's N x N `sim`, their sigmoid, and the
(roc_auc, avg_prec) it returned.  Plus two synthetic score / label sets for the ranking metrics alone -- one with saturated ties
(logits x 20: many probabilities are exactly 1.0f), one with all scores distinct -- whose sklearn values are recorded through the
reference's edge_predict_score."""
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
sys.path.insert(0, HERE)

import numpy as np
import scipy.sparse as sp
import torch

from inputs import hash_matrix, hash_positive  # noqa: E402

METHODS = ("mean", "max", "concat", "simple")
HOPS = (0, 1, 3, 6)
R_LIST = [0.5, 0.3, 0]


def graph(name):
    g = np.load(os.path.join(HERE, "graphs.npz"))
    indptr, indices, data = g[name + "|indptr"], g[name + "|indices"], g[name + "|data"]
    n = len(indptr) - 1
    return sp.csr_matrix((data, indices, indptr), shape=(n, n))


def reference_task_module():
    for m in ["matplotlib", "matplotlib.pyplot", "munkres"]:
        try:
            importlib.import_module(m)
        except ImportError:
            sys.modules[m] = MagicMock()
    if "sgl.tasks" not in sys.modules:
        pkg = types.ModuleType("sgl.tasks")
        pkg.__path__ = [REF + "/sgl/tasks"]
        sys.modules["sgl.tasks"] = pkg
    import sgl.tasks.link_prediction as lp
    return lp


def main():
    lp = reference_task_module()
    score = lp.edge_predict_score                    # sgl/tasks/utils.py:263-271 (sklearn inside)
    seen = {}

    def capturing(sim, pos, neg, thr):
        seen["sim"] = sim.clone()
        return score(sim, pos, neg, thr)

    lp.edge_predict_score = capturing
    g = graph("pl256")
    n = g.shape[0]
    x = hash_positive(n, 12, seed=41)
    rng = np.random.default_rng(14)
    coo = sp.triu(g, 1).tocoo()
    pick = rng.choice(coo.nnz, 200, replace=False)
    pos = np.stack((coo.row[pick], coo.col[pick]), 1).astype(np.int64)
    neg = rng.integers(0, n, (200, 2)).astype(np.int64)

    class DS:
        adj = g
        num_node = n
    DS.x = x

    out = {"x": x, "hops": np.array(HOPS), "r_list": np.array(R_LIST, dtype=np.float64), "pos_edges": pos, "neg_edges": neg}
    both = np.concatenate((pos, neg))
    for method in METHODS:
        for hops in HOPS:
            task = object.__new__(lp.LinkPredictionNAFS)
            task._LinkPredictionNAFS__dataset = DS
            task._LinkPredictionNAFS__train_adj = g
            task._LinkPredictionNAFS__r_list = list(R_LIST)
            task._LinkPredictionNAFS__method = method
            task._LinkPredictionNAFS__test_edges = torch.from_numpy(pos)
            task._LinkPredictionNAFS__test_edges_neg = torch.from_numpy(neg)
            task._LinkPredictionNAFS__pred_threshold = 0.5
            roc_auc, avg_prec = task._k_hop_link_prediction(hops)
            logits = seen["sim"][both[:, 0], both[:, 1]].reshape(-1)
            assert logits.dtype == torch.float32
            key = f"lp|{method}|hops{hops}"
            out[key + "|logits"] = logits.numpy().copy()
            out[key + "|probs"] = torch.sigmoid(logits).numpy().copy()
            out[key + "|metrics"] = np.array([roc_auc, avg_prec], dtype=np.float64)

    # the ranking metrics alone: a [1, M] `edge_feature` of logits, the "edges" (0, j) split by label
    m = 400
    base = hash_matrix(1, m, seed=1414)[0].astype(np.float64)
    sets = {"ties": (base * 3.0 * 20.0).astype(np.float32),                       # |logit| up to 60: sigmoid saturates at 1.0f
            "distinct": (np.linspace(-4.0, 4.0, m)[rng.permutation(m)]).astype(np.float32)}
    for name, logits in sets.items():
        labels = (rng.random(m) < 0.45)
        feat = torch.from_numpy(logits)[None, :]
        cols = np.arange(m, dtype=np.int64)
        p_e = np.stack((np.zeros(int(labels.sum()), np.int64), cols[labels]), 1)
        n_e = np.stack((np.zeros(int((~labels).sum()), np.int64), cols[~labels]), 1)
        roc_auc, avg_prec = score(feat, torch.from_numpy(p_e), torch.from_numpy(n_e), 0.5)
        probs = torch.sigmoid(torch.cat((feat[0, p_e[:, 1]], feat[0, n_e[:, 1]]))).numpy().copy()
        if name == "ties":
            assert (probs == 1.0).sum() > 20 and len(np.unique(probs)) < m
        else:
            assert len(np.unique(probs)) == m
        out[f"metrics|{name}|probs"] = probs
        out[f"metrics|{name}|labels"] = np.concatenate((np.ones(len(p_e), np.float32), np.zeros(len(n_e), np.float32)))
        out[f"metrics|{name}|metrics"] = np.array([roc_auc, avg_prec], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "g14_link_prediction.npz"), **out)


if __name__ == "__main__":
    main()

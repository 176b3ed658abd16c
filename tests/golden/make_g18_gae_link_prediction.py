#!/usr/bin/env python3
"""Generate tests/golden/g18_gae_link_prediction.npz by IMPORTING THE REFERENCE ITSELF (as make_g14_link_prediction.py does).

    PYTHONDONTWRITEBYTECODE=1 SGL_REFERENCE=<checkout of the reference> python tests/golden/make_g18_gae_link_prediction.py

Needs the reference and sklearn (what its edge_predict_train / edge_predict_score call); nothing of the reference travels: the
fixture holds inputs and recorded outputs only.

G18, on graph pl256 with Z = hash_matrix(256, 12), 200 positive pairs taken from the graph and 200 seeded random pairs:
  train|*   the reference's own edge_predict_train (sgl/tasks/utils.py:274-303) with its default loss_fn
            (F.binary_cross_entropy_with_logits, sgl/tasks/link_prediction.py:15), driven by a stub model whose model_forward returns
            a leaf nn.Parameter holding Z and by SGD with lr = 0: loss, Z.grad, roc_auc, avg_prec; and the same loss and gradient in
            float64, by re-running the reference's expression on Z.double()
  eval|*    edge_predict_eval's four numbers for that model (val = the first 100 of each list, test = the rest)
  task|*    three epochs of LinkPredictionGAE._execute (sgl/tasks/link_prediction.py:81-157) with an SGC-like model -- one Linear
            layer on x = two hops of the symmetrically normalised graph applied to hash_matrix(256, 12, seed=19) -- from the saved
            state_dict, lr = 0.01: per-epoch loss, the final logits of the test edges against all negatives, and the returned pair;
            the same run in float64 (model.double(), x.double())."""
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
sys.path.insert(0, HERE)

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as F

from inputs import hash_matrix  # noqa: E402

D, HIDDEN, EPOCHS, LR = 12, 8, 3, 0.01


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


class Stub(nn.Module):
    """model_forward returns a leaf parameter: its .grad is dLoss / dZ"""

    def __init__(self, z):
        super().__init__()
        self.z = nn.Parameter(z.clone())

    def model_forward(self, idx, device):
        return self.z


def sgc_model(base, f_in, dtype):
    """one Linear layer on the pre-propagated features: BaseSGAPModel without graph operators"""
    class SGCLike(base):
        def __init__(self):
            super().__init__(2, f_in, HIDDEN)
            self._base_model = nn.Linear(f_in, HIDDEN).to(dtype)
    return SGCLike()


def main():
    lp = reference_task_module()
    import sgl.tasks.utils as ut
    for m in ["torch_geometric", "torch_geometric.data", "torch_geometric.datasets", "torch_geometric.io", "torch_geometric.utils",
              "torch_sparse", "ogb", "ogb.nodeproppred", "gensim", "gensim.models", "openbox"]:
        sys.modules.setdefault(m, MagicMock())       # what the reference's dataset modules import and a model without operators never uses
    import sgl.dataset  # noqa: F401  (must come first: circular import)
    from sgl.models.base_model import BaseSGAPModel
    g = graph("pl256")
    n = g.shape[0]
    z = hash_matrix(n, D)
    rng = np.random.default_rng(18)
    coo = sp.triu(g, 1).tocoo()
    pick = rng.choice(coo.nnz, 200, replace=False)
    pos = np.stack((coo.row[pick], coo.col[pick]), 1).astype(np.int64)
    neg = rng.integers(0, n, (200, 2)).astype(np.int64)
    tpos, tneg = torch.from_numpy(pos), torch.from_numpy(neg)
    out = {"z": z, "pos_edges": pos, "neg_edges": neg}
    cpu = torch.device("cpu")

    # ---- one training step of the reference, float32, and its expression in float64
    model = Stub(torch.from_numpy(z))
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    loss, roc_auc, avg_prec = ut.edge_predict_train(model, None, True, tpos, tneg, cpu, opt, F.binary_cross_entropy_with_logits, 0.5)
    out["train|loss"] = np.array(loss, dtype=np.float64)
    out["train|grad"] = model.z.grad.numpy().copy()
    out["train|metrics"] = np.array([roc_auc, avg_prec], dtype=np.float64)
    z64 = torch.from_numpy(z).double().requires_grad_(True)
    edges = torch.cat((tpos, tneg))
    labels = torch.cat((torch.ones(len(pos)), torch.zeros(len(neg)))).double()
    pred = torch.sigmoid(torch.mm(z64, z64.t())[edges[:, 0], edges[:, 1]].reshape(-1))
    loss64 = F.binary_cross_entropy_with_logits(pred, labels)
    loss64.backward()
    out["train|loss64"] = np.array(loss64.item(), dtype=np.float64)
    out["train|grad64"] = z64.grad.numpy().copy()
    # the loss people mean -- the same loss_fn on the logits themselves, i.e. the reference's expression without its torch.sigmoid line
    for tag, dtype in (("", torch.float32), ("64", torch.float64)):
        zz = torch.from_numpy(z).to(dtype).requires_grad_(True)
        logits = torch.mm(zz, zz.t())[edges[:, 0], edges[:, 1]].reshape(-1)
        loss_l = F.binary_cross_entropy_with_logits(logits, labels.to(dtype))
        loss_l.backward()
        out["train_logits|loss" + tag] = np.array(loss_l.item(), dtype=np.float64)
        out["train_logits|grad" + tag] = zz.grad.numpy().copy()
    out["eval|metrics"] =np.array(ut.edge_predict_eval(model, None, tpos[:100], tneg[:100], tpos[100:], tneg[100:], cpu, 0.5), dtype=np.float64)

    # ---- three epochs of the task
    deg = np.asarray(g.sum(1)).reshape(-1)
    dinv = sp.diags(np.where(deg > 0, deg ** -0.5, 0.0))
    norm = (dinv @ g @ dinv).tocsr()
    x = np.ascontiguousarray((norm @ (norm @ hash_matrix(n, D, seed=19).astype(np.float64))).astype(np.float32))
    out["task|x"] = x
    split = {"train": (pos[:140], neg[:140]), "val": (pos[140:160], neg[140:160]), "test": (pos[160:], neg[160:])}
    torch.manual_seed(18)
    state = {k: v.clone() for k, v in sgc_model(BaseSGAPModel, D, torch.float32).state_dict().items()}
    for k, v in state.items():
        out["task|state|" + k] = v.numpy().copy()
    out["task|epochs"], out["task|lr"] = np.array(EPOCHS), np.array(LR)
    train = ut.edge_predict_train

    class DS:
        adj = g
        num_node = n

    for tag, dtype in (("", torch.float32), ("64", torch.float64)):
        model = sgc_model(BaseSGAPModel, D, dtype)
        model.load_state_dict({k: v.to(dtype) for k, v in state.items()})
        DS.x = torch.from_numpy(x).to(dtype)
        losses = []

        def recording(*a, **kw):
            r = train(*a, **kw)
            losses.append(r[0])
            return r

        lp.edge_predict_train = recording
        task = object.__new__(lp.LinkPredictionGAE)
        p = "_LinkPredictionGAE__"
        for name, value in (("dataset", DS), ("edge_labels", torch.zeros(1)), ("train_adj", g), ("model", model), ("with_params", True),
                            ("optimizer", torch.optim.Adam(model.parameters(), lr=LR, weight_decay=0.0)), ("epochs", EPOCHS),
                            ("loss_fn", F.binary_cross_entropy_with_logits), ("device", cpu), ("seed", 42), ("pred_threshold", 0.5),
                            ("mini_batch", False)):
            setattr(task, p + name, value)
        for name, (a, b) in split.items():
            setattr(task, p + name + "_edges", torch.from_numpy(a))
            setattr(task, p + name + "_edges_neg", torch.from_numpy(b))
        all_neg = torch.cat([torch.from_numpy(split[s][1]) for s in ("train", "val", "test")])
        setattr(task, p + "all_edges_neg", all_neg)
        pair = task._execute()
        lp.edge_predict_train = train
        model.eval()
        with torch.no_grad():
            zf = model.model_forward(torch.arange(n), cpu)
            scored = torch.cat((torch.from_numpy(split["test"][0]), all_neg))
            logits = torch.mm(zf, zf.t())[scored[:, 0], scored[:, 1]].reshape(-1)
        out["task|loss" + tag] = np.array(losses, dtype=np.float64)
        out["task|logits" + tag] = logits.numpy().copy()
        out["task|pair" + tag] = np.array(pair, dtype=np.float64)
    for name, (a, b) in split.items():
        out[f"task|{name}_edges"], out[f"task|{name}_edges_neg"] = a, b
    np.savez_compressed(os.path.join(HERE, "g18_gae_link_prediction.npz"), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})
    print(out["train|loss"], out["train|loss64"], out["train|metrics"], out["eval|metrics"], out["task|loss"], out["task|loss64"], out["task|pair"],
          out["task|pair64"])


if __name__ == "__main__":
    main()

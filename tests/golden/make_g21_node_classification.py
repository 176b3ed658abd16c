#!/usr/bin/env python3
"""Generate tests/golden/g21_node_classification.npz by IMPORTING THE REFERENCE ITSELF (as make_g18_gae_link_prediction.py and
make_g19_node_clustering_train.py do).

    PYTHONDONTWRITEBYTECODE=1 SGL_REFERENCE=<checkout of the reference> python tests/golden/make_g21_node_classification.py

Needs the reference, sklearn and scipy (its task modules import them); nothing of the reference travels: the fixture holds inputs and
recorded outputs only.  Everything is recorded in float32 and in float64 (the same float32 inputs, widened).

G21 holds four things.
(a) step|*  a logits matrix [96, 7] (rows of scale 0.1 / 1 / 8 / 40 and offset 0 / 1e4 / -3e3, as tests/class_loss_common.py draws
    them) and labels with every 17th row -100, with the loss and the .grad of a leaf of nn.CrossEntropyLoss() and of the reference's
    LogeCrossEntropy (sgl/tricks/utils.py:7-10).
(b) acc|*   the reference's accuracy (sgl/tasks/utils.py:12-16) on rows that include exact ties of two and three maxima.
(c) loop|*  a stub model whose model_forward is a seeded Linear(12, 5) over a fixed feature matrix [150, 12]: three epochs of the
    reference's train + evaluate (full|*), then, from the same initial state, three epochs of mini_batch_train + mini_batch_evaluate
    over explicit batch lists (mini|*: 4 training batches of 20, evaluation batches of 32); Adam(lr = 0.05).  Recorded: per-epoch
    loss and accuracies, the final weights.  Both with nn.CrossEntropyLoss() and (full only) LogeCrossEntropy.
(d) task|*  NodeClassification._execute (sgl/tasks/node_classification.py:45-112) on a stub dataset with the same model, whose
    postprocess(adj, output) is adj @ output for a stored dense row-normalised matrix: per-epoch values, the post-processing
    accuracies, best val / best test."""
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
import torch
import torch.nn as nn
from scipy.optimize import linear_sum_assignment

N, F_IN, CLASSES, EPOCHS, LR = 150, 12, 5, 3, 0.05
TRAIN, VAL = 80, 35                                # the first 80 nodes train, the next 35 validate, the rest test


class Munkres:
    """stand-in for munkres.Munkres (imported by the reference's clustering metrics, not used here)"""

    def compute(self, cost):
        rows, cols = linear_sum_assignment(np.asarray(cost))
        return list(zip(rows.tolist(), cols.tolist()))


def reference_modules():
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
    for name in ("tasks", "tricks"):                 # the packages' own __init__ import every task / trick and what those need
        if "sgl." + name not in sys.modules:
            pkg = types.ModuleType("sgl." + name)
            pkg.__path__ = [REF + "/sgl/" + name]
            sys.modules["sgl." + name] = pkg
    import sgl.tasks.node_classification as nc
    import sgl.tasks.utils as ut
    import sgl.tricks.utils as tu
    return nc, ut, tu


class Stub(nn.Module):
    """model_forward = a Linear layer over the rows of a fixed feature matrix; postprocess = a fixed matrix applied to the output"""

    def __init__(self, x, dtype):
        super().__init__()
        self.lin = nn.Linear(F_IN, CLASSES).to(dtype)
        self.x = x.to(dtype)

    def preprocess(self, adj, x):
        pass

    def model_forward(self, idx, device):
        return self.lin(self.x[torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx, dtype=torch.long)])

    def postprocess(self, adj, output):
        return adj.to(output.dtype) @ output


def main():
    nc, ut, tu = reference_modules()
    out = {}
    # ---- (a) one loss and its gradient
    rng = np.random.default_rng(2121)
    n, c = 96, 7
    z = (rng.standard_normal((n, c)) * rng.choice([0.1, 1.0, 8.0, 40.0], (n, 1)) + rng.choice([0.0, 0.0, 1e4, -3e3], (n, 1))).astype(np.float32)
    y = rng.integers(0, c, n).astype(np.int64)
    y[::17] = -100
    out["step|z"], out["step|labels"] = z, y
    for name, fn in (("ce", nn.CrossEntropyLoss()), ("loge", tu.LogeCrossEntropy)):
        for tag, dtype in (("", torch.float32), ("64", torch.float64)):
            leaf = torch.from_numpy(z).to(dtype).requires_grad_(True)
            loss = fn(leaf, torch.from_numpy(y))
            loss.backward()
            out[f"step|{name}|loss{tag}"] = np.array(float(loss.detach()), dtype=np.float64)
            out[f"step|{name}|grad{tag}"] = leaf.grad.numpy().copy()
        print("step", name, out[f"step|{name}|loss"], out[f"step|{name}|loss64"])

    # ---- (b) accuracy with exact ties
    t = rng.permutation(40 * 6).reshape(40, 6).astype(np.float32)
    for i in range(0, 40, 4):
        cols = rng.choice(6, 3, replace=False)
        t[i, cols[:2]] = t[i].max() + 1
        t[i + 1, cols] = t[i + 1].max() + 1
    ty = torch.from_numpy(t).max(1)[1].numpy().copy()
    ty[::3] = (ty[::3] + 1) % 6
    out["acc|z"], out["acc|labels"] = t, ty.astype(np.int64)
    out["acc|value"] = np.array(ut.accuracy(torch.from_numpy(t), torch.from_numpy(ty)), dtype=np.float64)
    out["acc|pred"] = torch.from_numpy(t).max(1)[1].numpy()
    print("acc", out["acc|value"])

    # ---- (c) the loops
    centres = rng.standard_normal((CLASSES, F_IN)) * 1.2
    labels = rng.integers(0, CLASSES, N).astype(np.int64)
    x = (centres[labels] + rng.standard_normal((N, F_IN))).astype(np.float32)
    labels = np.where(rng.random(N) < 0.1, rng.integers(0, CLASSES, N), labels).astype(np.int64)
    train_idx, val_idx, test_idx = np.arange(TRAIN), np.arange(TRAIN, TRAIN + VAL), np.arange(TRAIN + VAL, N)
    perm = rng.permutation(TRAIN)
    train_batches = [perm[i:i + 20].astype(np.int64) for i in range(0, TRAIN, 20)]
    val_batches = [val_idx[i:i + 32] for i in range(0, len(val_idx), 32)]
    test_batches = [test_idx[i:i + 32] for i in range(0, len(test_idx), 32)]
    post = (rng.random((N, N)) < 0.05).astype(np.float64) + np.eye(N)
    post = (post / post.sum(1, keepdims=True)).astype(np.float32)
    out.update({"loop|x": x, "loop|y": labels, "loop|train_idx": train_idx, "loop|val_idx": val_idx, "loop|test_idx": test_idx,
                "loop|train_batches": np.stack(train_batches), "loop|eval_batch": np.array(32), "loop|epochs": np.array(EPOCHS),
                "loop|lr": np.array(LR), "task|post": post})
    torch.manual_seed(21)
    state = {key: v.clone() for key, v in Stub(torch.from_numpy(x), torch.float32).state_dict().items()}
    for key, v in state.items():
        out["loop|state|" + key] = v.numpy().copy()
    cpu = torch.device("cpu")
    yt = torch.from_numpy(labels)

    def fresh(dtype):
        model = Stub(torch.from_numpy(x), dtype)
        model.load_state_dict({key: v.to(dtype) for key, v in state.items()})
        return model, torch.optim.Adam(model.parameters(), lr=LR, weight_decay=0.0)

    for tag, dtype in (("", torch.float32), ("64", torch.float64)):
        for name, fn in (("ce", nn.CrossEntropyLoss()), ("loge", tu.LogeCrossEntropy)):
            model, opt = fresh(dtype)
            rows = []
            for _ in range(EPOCHS):
                loss, acc = ut.train(model, train_idx, yt, cpu, opt, fn)
                rows.append((loss, acc) + tuple(ut.evaluate(model, val_idx, test_idx, yt, cpu)))
            out[f"full|{name}|history{tag}"] = np.array(rows, dtype=np.float64)          # loss, acc_train, acc_val, acc_test
            for key, v in model.state_dict().items():
                out[f"full|{name}|final{tag}|{key}"] = v.detach().numpy().copy()
        model, opt = fresh(dtype)
        rows = []
        for _ in range(EPOCHS):
            loss, acc = ut.mini_batch_train(model, train_idx, train_batches, yt, cpu, opt, nn.CrossEntropyLoss())
            rows.append((loss, acc) + tuple(ut.mini_batch_evaluate(model, val_idx, val_batches, test_idx, test_batches, yt, cpu)))
        out[f"mini|ce|history{tag}"] = np.array(rows, dtype=np.float64)
        for key, v in model.state_dict().items():
            out[f"mini|ce|final{tag}|{key}"] = v.detach().numpy().copy()
        print("full ce", out[f"full|ce|history{tag}"], "\nfull loge", out[f"full|loge|history{tag}"], "\nmini", out[f"mini|ce|history{tag}"])

        # ---- (d) the task
        class Data:
            num_node = N

        class DS:
            adj = torch.from_numpy(post)
            data = Data
            num_node = N
        DS.x, DS.y = torch.from_numpy(x).to(dtype), yt
        DS.train_idx, DS.val_idx, DS.test_idx = train_idx, val_idx, test_idx
        model, opt = fresh(dtype)
        seen = []
        real_train, real_eval = ut.train, ut.evaluate

        def rec_train(*a, **kw):
            r = real_train(*a, **kw)
            seen.append(("train",) + tuple(r))
            return r

        def rec_eval(*a, **kw):
            r = real_eval(*a, **kw)
            seen.append(("eval",) + tuple(r))
            return r

        nc.train, nc.evaluate = rec_train, rec_eval
        task = object.__new__(nc.NodeClassification)
        p = "_NodeClassification__"
        for attr, value in (("dataset", DS), ("labels", DS.y), ("model", model), ("optimizer", opt), ("epochs", EPOCHS),
                            ("loss_fn", nn.CrossEntropyLoss()), ("device", cpu), ("seed", 42), ("mini_batch", False)):
            setattr(task, p + attr, value)
        best_test = task._execute()
        post_val, post_test = task._postprocess()
        nc.train, nc.evaluate = real_train, real_eval
        hist = np.array([seen[2 * e][1:] + seen[2 * e + 1][1:] for e in range(EPOCHS)], dtype=np.float64)
        best_val = max([0.0] + [h[2] for h in hist] + [post_val])
        out[f"task|history{tag}"] = hist
        out[f"task|post{tag}|acc"] = np.array([post_val, post_test], dtype=np.float64)
        out[f"task|best{tag}"] = np.array([best_val, best_test], dtype=np.float64)
        print("task", hist, post_val, post_test, best_val, best_test)
    assert np.array_equal(out["task|history"][:, 1:], out["task|history64"][:, 1:]), "float32 and float64 runs predict differently: choose other data"
    assert np.array_equal(out["task|best"], out["task|best64"]) and np.array_equal(out["task|post|acc"], out["task|post64|acc"])
    for key in ("full|ce|history", "full|loge|history", "mini|ce|history"):
        assert np.array_equal(out[key][:, 1:], out[key + "64"][:, 1:]), key
    assert out["task|post|acc"][0] != out["task|history"][-1, 2] or out["task|post|acc"][1] != out["task|history"][-1, 3], "postprocess changes nothing"
    path = os.path.join(HERE, "g21_node_classification.npz")
    np.savez_compressed(path, **out)
    print({key: (v.shape, v.dtype) for key, v in out.items()})
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

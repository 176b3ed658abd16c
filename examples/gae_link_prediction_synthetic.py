#!/usr/bin/env python3
"""The trainable link-prediction task (LinkPredictionGAE: mask_test_edges, then epochs of edge_predict_train / edge_predict_eval;
sgl/tasks/link_prediction.py:14-157) on the MI355X, on the device from end to end: the graph is generated there (a degree-corrected
planted partition), `mask_test_edges` splits its edges and draws the negative pairs there, an SGC-style model -- K hops of the
normalised training graph once, then one Linear layer -- is trained there by `gae_link_prediction`: per epoch the scores of all
training pairs are one launch, their loss E floats in torch, and its gradient one launch over the edge list grouped by endpoint once
(`EdgePlan`; no N x N matrix, no sort, no atomics).  No edge and no feature is copied to the host.

    python examples/gae_link_prediction_synthetic.py [--nodes 200000] [--edges 2000000] [--hops 2] [--hidden 64] [--epochs 5]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgl_amd import device as dev, synthetic  # noqa: E402
from sgl_amd.io import DeviceAdjacency  # noqa: E402
from sgl_amd.tricks import gae_link_prediction, mask_test_edges  # noqa: E402


class SGC(torch.nn.Module):
    """SGC with the reference's model interface: preprocess propagates once, model_forward is a Linear layer on the result"""

    def __init__(self, hops, f_in, hidden):
        super().__init__()
        self.hops = hops
        self._base_model = torch.nn.Linear(f_in, hidden)
        self.x = None

    def preprocess(self, adj, x):
        n = adj.shape[0]
        rowptr, col, val = dev.normalize_adj(adj.rowptr, adj.col, adj.val, n, 0.5)
        csr = dev.DeviceCSR(rowptr, col, val, (n, n))
        for _ in range(self.hops):
            x = csr.spmm(x)
        self.x = x

    def model_forward(self, idx, device):
        return self._base_model(self.x[idx])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--block", type=int, default=64, help="nodes per community")
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--activation", default="sigmoid", choices=("sigmoid", "none"), help="sigmoid: the reference as written")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    n = a.nodes
    rowptr, col, val, community = synthetic.planted_partition_torch(n, a.edges, 500, a.block, p_in=0.8, seed=a.seed, device=device)
    adj = DeviceAdjacency(rowptr, col, val, (n, n))
    g = torch.Generator(device=device)
    g.manual_seed(a.seed + 1)
    centres = torch.randn((int(community.max()) + 1, a.dim), generator=g, device=device)
    x = dev.alloc_rows(n, a.dim, device)
    x.copy_(0.5 * centres[community] + torch.randn((n, a.dim), generator=g, device=device))

    torch.cuda.synchronize()
    t0 = time.time()
    split = mask_test_edges(adj, seed=a.seed)
    torch.cuda.synchronize()
    t1 = time.time()
    torch.manual_seed(a.seed)
    model = SGC(a.hops, a.dim, a.hidden)
    res = gae_link_prediction(model, split, x, epochs=a.epochs, lr=a.lr, weight_decay=0.0, seed=a.seed, activation=a.activation)
    torch.cuda.synchronize()
    t2 = time.time()
    print(f"{n} nodes, {adj.nnz} stored entries: {len(split.train_edges)} train / {len(split.val_edges)} val / {len(split.test_edges)} test "
          f"edges and as many negative pairs each; split {t1 - t0:.3f} s, {a.hops} hops + {a.epochs} epochs {t2 - t1:.3f} s")
    print("epoch  loss     roc_auc_val  avg_prec_val  roc_auc_test  avg_prec_test")
    for h in res.history:
        loss = f"{h['loss']:.4f}" if "loss" in h else "      "
        print(f"{str(h['epoch']):>5}  {loss}   {h['roc_auc_val']:.4f}       {h['avg_prec_val']:.4f}        {h['roc_auc_test']:.4f}        "
              f"{h['avg_prec_test']:.4f}")
    print(f"kept: test roc_auc {res.test_roc_auc:.4f}, test avg_prec {res.test_avg_prec:.4f} (at the best validation scores; the last row "
          "scores the test edges against ALL negative pairs, as the reference's post-processing does)")
    losses = [h["loss"] for h in res.history[:-1]]
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0], losses


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The trainable node-clustering task (NodeClustering: epochs of clustering_train -- model_forward, KMeans of the output, cluster_loss,
backward, three scores -- then a final clustering step; sgl/tasks/node_clustering.py:12-119, sgl/tasks/utils.py:101-136) on the MI355X,
on the device from end to end: the graph is generated there (a degree-corrected planted partition with a few large blocks), the
features are planted blobs -- one centre per block under unit noise -- an SGC-style model (K hops of the normalised graph once, then
one Linear layer) is trained there by `node_clustering`: per epoch the k-means of the model output (assignment kernel + membership
SpMM), then the loss and its gradient in ONE launch (sgl_cluster_loss_grad_f32: one read of the output, one write of dX), then the
three scores from one contingency table.  No feature matrix, no model output and no label vector is copied to the host.

    python examples/node_clustering_synthetic.py [--nodes 200000] [--edges 2000000] [--classes 8] [--hops 2] [--hidden 64] [--epochs 5]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgl_amd import device as dev, synthetic  # noqa: E402
from sgl_amd.io import DeviceAdjacency  # noqa: E402
from sgl_amd.tricks import node_clustering  # noqa: E402


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
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--n-init", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    n = a.nodes
    block = -(-n // a.classes)
    rowptr, col, val, y = synthetic.planted_partition_torch(n, a.edges, 500, block, p_in=0.8, seed=a.seed, device=device)
    adj = DeviceAdjacency(rowptr, col, val, (n, n))
    g = torch.Generator(device=device)
    g.manual_seed(a.seed + 1)
    centres = torch.randn((int(y.max()) + 1, a.dim), generator=g, device=device)
    x = dev.alloc_rows(n, a.dim, device)
    x.copy_(centres[y] + torch.randn((n, a.dim), generator=g, device=device))

    torch.manual_seed(a.seed)
    model = SGC(a.hops, a.dim, a.hidden)
    torch.cuda.synchronize()
    t0 = time.time()
    res = node_clustering(model, adj, x, y, epochs=a.epochs, lr=a.lr, weight_decay=0.0, n_init=a.n_init, seed=a.seed, device=device)
    torch.cuda.synchronize()
    took = time.time() - t0
    print(f"{n} nodes, {adj.nnz} stored entries, {a.classes} blocks, output width {a.hidden}: {a.hops} hops + {a.epochs} epochs + the final "
          f"step (k-means with n_init {a.n_init} each) {took:.3f} s")
    print("epoch  loss      acc     nmi     adjscore")
    for h in res.history:
        loss = f"{h['loss']:8.4f}" if "loss" in h else "        "
        print(f"{str(h['epoch']):>5}  {loss}  {h['acc']:.4f}  {h['nmi']:.4f}  {h['adjscore']:.4f}")
    print(f"best: acc {res.acc:.4f}, nmi {res.nmi:.4f}, adjscore {res.adjscore:.4f}")
    losses = [h["loss"] for h in res.history[:-1]]
    assert all(torch.isfinite(torch.tensor(losses))), losses
    assert res.adjscore > 0.5, "the planted blocks were not found"


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Inductive SGC: the model never sees a test node -- nor an edge that touches one -- while it trains.  The sub-graph of the training
nodes is cut out ON THE DEVICE (sgl_amd.transforms.get_subgraph: one stable compaction of the resident CSR; the
reference's get_subgraph goes through a COO edge list and a new scipy matrix on the host), SGC is pre-propagated and trained on it,
then pre-propagated again on the whole graph and scored on the test nodes.  The graph, features and labels are synthetic (planted
communities, as in sgc_synthetic.py).

    python examples/inductive_sgc_synthetic.py [--nodes 19717 --feat 500 --classes 3 --epochs 50 --train-share 0.4]"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgc_synthetic import planted_graph  # noqa: E402
from sgl_amd import transforms  # noqa: E402
from sgl_amd.io import DeviceAdjacency  # noqa: E402
from sgl_amd.models.homo import SGC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=19717)
    ap.add_argument("--feat", type=int, default=500)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--prop-steps", type=int, default=3)
    ap.add_argument("--train-share", type=float, default=0.4)
    a = ap.parse_args()
    device = torch.device("cuda")
    graph, y = planted_graph(a.nodes, a.classes, 8, 0.8, seed=0)
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((a.nodes, a.feat)) + 0.35 * np.eye(a.classes)[y] @ rng.standard_normal((a.classes, a.feat))).astype(np.float32)
    adj = DeviceAdjacency.from_scipy(graph, device=device)        # uploaded once; everything below stays on the device
    x = torch.from_numpy(x).to(device)
    labels = torch.from_numpy(y).to(device)
    train_mask = torch.from_numpy(rng.random(a.nodes) < a.train_share).to(device)
    test_idx = torch.nonzero(~train_mask).reshape(-1)

    torch.cuda.synchronize()
    t0 = time.time()
    sub = transforms.get_subgraph(adj, train_mask, x=x, y=labels)
    torch.cuda.synchronize()
    k = sub.adj.shape[0]
    print(f"Training sub-graph: {k} of {a.nodes} nodes, {sub.adj.nnz} of {adj.nnz} entries, cut out in {time.time() - t0:.4f}s")
    assert k == int(train_mask.sum()) and sub.x.shape == (k, a.feat) and torch.equal(sub.y, labels[train_mask])

    model = SGC(prop_steps=a.prop_steps, feat_dim=a.feat, output_dim=a.classes).to(device)
    t0 = time.time()
    model.preprocess(sub.adj, sub.x)              # the training nodes and the edges among them: nothing of a test node
    torch.cuda.synchronize()
    print(f"Preprocessing of the sub-graph done in {time.time() - t0:.4f}s")
    opt = torch.optim.Adam(model.parameters(), lr=0.1, weight_decay=5e-5)
    rows = range(k)
    for epoch in range(a.epochs):
        model.train()
        opt.zero_grad()
        loss = F.cross_entropy(model.model_forward(rows, device), sub.y)
        loss.backward()
        opt.step()
    model.eval()
    t0 = time.time()
    model.preprocess(adj, x)                      # inference: the whole graph, the weights trained on the sub-graph
    torch.cuda.synchronize()
    print(f"Preprocessing of the whole graph done in {time.time() - t0:.4f}s")
    with torch.no_grad():
        acc = (model.model_forward(test_idx, device).argmax(1) == labels[test_idx]).float().mean().item()
    print(f"epochs {a.epochs}  train loss {loss.item():.4f}  test acc {acc:.4f} on {test_idx.numel()} nodes never seen in training")
    assert acc > 1.5 / a.classes, "inductive SGC failed to learn the planted communities"


if __name__ == "__main__":
    main()

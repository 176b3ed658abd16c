#!/usr/bin/env python3
"""From a DIRECTED edge list to a trained SGC without leaving the device: the dump holds every edge of a planted-community graph in
one random direction only (what a citation dump such as ogbn-papers100M looks like); it is ingested as it is, symmetrised with
sgl_amd.transforms.to_undirected and given self-loops with add_self_loops -- both a merge of sorted rows of the resident CSR
(device.csr_merge; the reference stacks the COO list with its mirror on the host and builds a new scipy matrix) --
then propagated with LaplacianGraphOp on the DeviceAdjacency and trained as SGC.  The graph, features and labels are synthetic (as in
sgc_synthetic.py).

    python examples/undirected_sgc_synthetic.py [--nodes 19717 --feat 500 --classes 3 --epochs 50]"""
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
from sgl_amd.io import coo_to_csr_device  # noqa: E402
from sgl_amd.models.homo import SGC  # noqa: E402
from sgl_amd.operators.graph_op import LaplacianGraphOp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=19717)
    ap.add_argument("--feat", type=int, default=500)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--prop-steps", type=int, default=3)
    a = ap.parse_args()
    device = torch.device("cuda")
    graph, y = planted_graph(a.nodes, a.classes, 8, 0.8, seed=0)
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((a.nodes, a.feat)) + 0.35 * np.eye(a.classes)[y] @ rng.standard_normal((a.classes, a.feat))).astype(np.float32)
    upper = graph.tocoo()
    pick = upper.row < upper.col
    row, col = upper.row[pick], upper.col[pick]
    flip = rng.random(len(row)) < 0.5                              # every edge once, in a random direction: the directed dump
    row, col = np.where(flip, col, row), np.where(flip, row, col)
    x = torch.from_numpy(x).to(device)
    labels = torch.from_numpy(y).to(device)

    directed = coo_to_csr_device(row, col, np.ones(len(row), dtype=np.float32), a.nodes, device=device)
    torch.cuda.synchronize()
    t0 = time.time()
    adj = transforms.to_undirected(directed)                       # "sum", the reference's rule; no pair is stored both ways here
    torch.cuda.synchronize()
    t1 = time.time()
    looped = transforms.add_self_loops(adj)
    torch.cuda.synchronize()
    t2 = time.time()
    print(f"Directed dump: {directed.nnz} entries; to_undirected -> {adj.nnz} in {t1 - t0:.4f}s; add_self_loops -> {looped.nnz} in {t2 - t1:.4f}s")
    same = graph.tocsr()
    same.sort_indices()
    assert adj.nnz == 2 * directed.nnz == same.nnz and looped.nnz == adj.nnz + a.nodes
    assert np.array_equal(adj.col.cpu().numpy(), same.indices) and np.array_equal(adj.rowptr.cpu().numpy(), same.indptr)     # the graph itself again

    t0 = time.time()
    hops = LaplacianGraphOp(a.prop_steps).propagate(looped, x)
    torch.cuda.synchronize()
    print(f"LaplacianGraphOp({a.prop_steps}).propagate on the device adjacency: {len(hops)} hop matrices in {time.time() - t0:.4f}s")

    model = SGC(prop_steps=a.prop_steps, feat_dim=a.feat, output_dim=a.classes).to(device)
    t0 = time.time()
    model.preprocess(looped, x)
    torch.cuda.synchronize()
    print(f"Preprocessing done in {time.time() - t0:.4f}s")
    idx = rng.permutation(a.nodes)
    train_idx, test_idx = torch.from_numpy(idx[:a.nodes // 2]).to(device), torch.from_numpy(idx[a.nodes // 2:]).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=0.1, weight_decay=5e-5)
    for epoch in range(a.epochs):
        model.train()
        opt.zero_grad()
        loss = F.cross_entropy(model.model_forward(train_idx, device), labels[train_idx])
        loss.backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        acc = (model.model_forward(test_idx, device).argmax(1) == labels[test_idx]).float().mean().item()
    print(f"epochs {a.epochs}  train loss {loss.item():.4f}  test acc {acc:.4f} on {test_idx.numel()} nodes")
    assert acc > 1.5 / a.classes, "SGC on the symmetrised graph failed to learn the planted communities"


if __name__ == "__main__":
    main()

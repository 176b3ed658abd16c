#!/usr/bin/env python3
"""A composite relation of a heterogeneous graph as the input of a homogeneous model, without leaving the device: a synthetic paper /
author / field graph whose papers carry planted classes (authors write mostly inside one class), the relation
paper__to__author__to__paper through HeteroNodeDataset.sample_by_meta_path -- a sparse x sparse product on the device
(device.csr_matmul; the reference forms it with scipy on the host) -- then SGC.preprocess on the co-authorship graph
and a short training run on the papers.

    python examples/meta_path_sgc_synthetic.py [--papers 20000 --authors 12000 --fields 50 --feat 64 --classes 4 --epochs 50]"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgl_amd.hetero import HeteroGraph, HeteroNodeDataset  # noqa: E402
from sgl_amd.models.homo import SGC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--papers", type=int, default=20000)
    ap.add_argument("--authors", type=int, default=12000)
    ap.add_argument("--fields", type=int, default=50)
    ap.add_argument("--feat", type=int, default=64)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=50)
    a = ap.parse_args()
    device = torch.device("cuda")
    rng = np.random.default_rng(0)
    node_types, num = ["paper", "author", "field"], {"paper": a.papers, "author": a.authors, "field": a.fields}
    offset = {"paper": 0, "author": a.papers, "field": a.papers + a.authors}
    y = rng.integers(0, a.classes, a.papers)
    author_class = rng.integers(0, a.classes, a.authors)
    by_class = [np.nonzero(author_class == c)[0] for c in range(a.classes)]
    paper = np.repeat(np.arange(a.papers), 3)                       # three authors per paper, 80 % of them from the paper's class
    author = np.where(rng.random(paper.size) < 0.8, np.array([by_class[c][rng.integers(0, len(by_class[c]))] for c in y[paper]]),
                      rng.integers(0, a.authors, paper.size))
    field = rng.integers(0, a.fields, a.papers)
    rows = {"paper__to__author": paper + offset["paper"], "author__to__paper": author + offset["author"],
            "paper__to__field": np.arange(a.papers) + offset["paper"]}
    cols = {"paper__to__author": author + offset["author"], "author__to__paper": paper + offset["paper"], "paper__to__field": field + offset["field"]}
    edge_types = list(rows)
    x = {t: rng.standard_normal((num[t], a.feat)).astype(np.float32) for t in node_types}      # noise: the classes are in the structure alone
    x["paper"] += (0.15 * np.eye(a.classes)[y] @ rng.standard_normal((a.classes, a.feat))).astype(np.float32)
    graph = HeteroGraph(rows, cols, {e: np.ones(len(rows[e]), np.float32) for e in edge_types}, num, node_types, edge_types, x_dict=x,
                        y_dict={"paper": y}, device=device)
    ds = HeteroNodeDataset(graph)

    torch.cuda.synchronize()
    t0 = time.time()
    adj, feats, node_id = ds.sample_by_meta_path("paper__to__author__to__paper")
    torch.cuda.synchronize()
    print(f"paper__to__author__to__paper: {adj.shape[0]} papers, {adj.nnz} co-authorship entries in {time.time() - t0:.4f}s")
    assert adj.shape == (a.papers, a.papers) and node_id.tolist() == graph.node_id_dict["paper"] and bool((adj.val == 1.0).all())

    model = SGC(prop_steps=2, feat_dim=a.feat, output_dim=a.classes).to(device)
    model.preprocess(adj, feats)
    labels = torch.from_numpy(y).to(device)
    idx = rng.permutation(a.papers)
    train_idx, test_idx = torch.from_numpy(idx[:a.papers // 2]).to(device), torch.from_numpy(idx[a.papers // 2:]).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=0.05, weight_decay=5e-5)
    for epoch in range(a.epochs):
        model.train()
        opt.zero_grad()
        loss = F.cross_entropy(model.model_forward(train_idx, device), labels[train_idx])
        loss.backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        acc = (model.model_forward(test_idx, device).argmax(1) == labels[test_idx]).float().mean().item()
    print(f"epochs {a.epochs}  train loss {loss.item():.4f}  test acc {acc:.4f} on {test_idx.numel()} papers")
    assert acc > 1.5 / a.classes, "SGC on the co-authorship graph failed to learn the planted classes"


if __name__ == "__main__":
    main()

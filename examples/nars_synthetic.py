#!/usr/bin/env python3
"""NARS on a generated heterogeneous graph, on the MI355X from end to end (HeteroNodeClassification, sgl/tasks/node_classification.py:
115-217; NARS_SIGN and Fast_NARS_SGC_WithLearnableWeights, sgl/models/hetero): papers, authors and venues with planted classes, five
edge types (one inside a type, one stored in both directions); relation sub-graphs are drawn under a seed, built and propagated on the
device, and every training step reads its rows from all S * (K + 1) propagated matrices in one launch of the ensemble kernel (K16).

    python examples/nars_synthetic.py [--papers 60000] [--authors 40000] [--venues 500] [--dim 64] [--classes 8] [--hops 2]
                                      [--subgraphs 4] [--epochs 20] [--batch 8192]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgl_amd.hetero import HeteroGraph, HeteroNodeDataset  # noqa: E402
from sgl_amd.models.hetero import NARS_SIGN, Fast_NARS_SGC_WithLearnableWeights  # noqa: E402
from sgl_amd.tricks import hetero_node_classification  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--papers", type=int, default=60_000)
    ap.add_argument("--authors", type=int, default=40_000)
    ap.add_argument("--venues", type=int, default=500)
    ap.add_argument("--degree", type=int, default=6)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--subgraphs", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    g = torch.Generator(device=device)
    g.manual_seed(a.seed)
    num = {"paper": a.papers, "author": a.authors, "venue": a.venues}
    types = list(num)
    offset, count = {}, 0
    for t in types:
        offset[t] = count
        count += num[t]
    klass = {t: torch.randint(0, a.classes, (num[t],), generator=g, device=device) for t in types}
    centres = torch.randn((a.classes, a.dim), generator=g, device=device) * 0.5
    x = {t: centres[klass[t]] + torch.randn((num[t], a.dim), generator=g, device=device) for t in types}

    def edges(src, dst, per_node):
        """per_node edges from every src node; four in five end at a node of the source's class"""
        r = torch.arange(num[src], device=device).repeat_interleave(per_node)
        c = torch.randint(0, num[dst], (r.numel(),), generator=g, device=device)
        order = torch.argsort(klass[dst])
        first = torch.searchsorted(klass[dst][order], torch.arange(a.classes + 1, device=device))
        size = (first[1:] - first[:-1]).clamp(min=1)
        same = first[klass[src][r]] + (torch.rand(r.numel(), generator=g, device=device) * size[klass[src][r]]).long()
        c = torch.where(torch.rand(r.numel(), generator=g, device=device) < 0.8, order[same.clamp(max=num[dst] - 1)], c)
        return r + offset[src], c + offset[dst]

    rows, cols = {}, {}
    rows["paper__to__author"], cols["paper__to__author"] = edges("paper", "author", a.degree // 2)
    rows["author__to__paper"], cols["author__to__paper"] = cols["paper__to__author"], rows["paper__to__author"]     # the same relation, reversed
    rows["paper__to__paper"], cols["paper__to__paper"] = edges("paper", "paper", a.degree)
    rows["paper__to__venue"], cols["paper__to__venue"] = edges("paper", "venue", 1)
    rows["author__to__venue"], cols["author__to__venue"] = edges("author", "venue", 2)
    edge_types = list(rows)
    graph = HeteroGraph(rows, cols, {e: None for e in edge_types}, num, types, edge_types, None, x, {"paper": klass["paper"]}, device=device)
    order = torch.randperm(a.papers, generator=g, device=device)
    dataset = HeteroNodeDataset(graph, order[:a.papers // 10], order[a.papers // 10:a.papers // 5], order[a.papers // 5:])
    print(f"{count} nodes of {len(types)} types, {sum(int(r.numel()) for r in rows.values())} edges of {len(edge_types)} types")

    runs = ((NARS_SIGN, {}), (Fast_NARS_SGC_WithLearnableWeights, dict(train_batch_size=a.batch, eval_batch_size=4 * a.batch, record_subgraph_weight=True)))
    for cls, kw in runs:
        torch.manual_seed(a.seed)
        model = cls(a.hops, a.dim, a.classes, 128, 2, a.subgraphs)
        torch.cuda.synchronize()
        t0 = time.time()
        res = hetero_node_classification(model, dataset, "paper", epochs=a.epochs, lr=a.lr, weight_decay=0.0, seed=a.seed,
                                         random_subgraph_num=a.subgraphs, subgraph_edge_type_num=2, device=device, **kw)
        torch.cuda.synchronize()
        print(f"{cls.__name__}: best val {res.best_val:.4f}, test {res.best_test:.4f}, {time.time() - t0:.2f} s for preprocess + {a.epochs} epochs")
        if res.subgraph_weight is not None:
            print("  sub-graph weights at the best epoch:", [round(float(w), 3) for w in res.subgraph_weight])


if __name__ == "__main__":
    main()

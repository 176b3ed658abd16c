#!/usr/bin/env python3
"""The NAFS link-prediction task (LinkPredictionNAFS: mask_test_edges, then per hop count the NAFS features of the training graph and
the ROC-AUC / AP of the held-out edges against sampled non-edges; sgl/tasks/link_prediction.py:159-284) on the MI355X, on the device
from end to end: the graph is generated there (a degree-corrected planted partition), `mask_test_edges` splits its edges and draws
the negative pairs there, `nafs_link_prediction` propagates, scores and ranks there.  Two floats per hop count come back.

    python examples/nafs_link_prediction_split.py [--nodes 200000] [--edges 2000000] [--hops 6] [--method mean] [--seed 0]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgl_amd import synthetic  # noqa: E402
from sgl_amd.io import DeviceAdjacency  # noqa: E402
from sgl_amd.tricks import has_edges, mask_test_edges, nafs_link_prediction  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--block", type=int, default=64, help="nodes per community")
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--hops", type=int, default=6)
    ap.add_argument("--method", default="mean", choices=("mean", "max", "concat", "simple"))
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    n = a.nodes
    rowptr, col, val, community = synthetic.planted_partition_torch(n, a.edges, 500, a.block, p_in=0.8, seed=a.seed, device=device)
    adj = DeviceAdjacency(rowptr, col, val, (n, n))
    # features: a weak trace of the node's community under unit noise
    g = torch.Generator(device=device)
    g.manual_seed(a.seed + 1)
    centres = torch.randn((int(community.max()) + 1, a.dim), generator=g, device=device)
    x = 0.5 * centres[community] + torch.randn((n, a.dim), generator=g, device=device)

    torch.cuda.synchronize()
    t0 = time.time()
    split = mask_test_edges(adj, seed=a.seed, negatives=("test",))                  # the task scores the test edges only
    torch.cuda.synchronize()
    t1 = time.time()
    assert bool(has_edges(adj, split.test_edges).all()) and not bool(has_edges(adj, split.test_edges_false).any())
    assert not bool(has_edges(split.adj_train, split.test_edges).any())
    res = nafs_link_prediction(split.adj_train, x, a.hops, split.test_edges, split.test_edges_false, r_list=(0.5, 0.3, 0), method=a.method,
                               device=device)
    torch.cuda.synchronize()
    t2 = time.time()
    print(f"{n} nodes, {adj.nnz} stored entries: {len(split.train_edges)} train / {len(split.val_edges)} val / {len(split.test_edges)} test "
          f"edges, {len(split.test_edges_false)} negative pairs; split {t1 - t0:.3f} s, {a.hops} hop counts ({a.method}) {t2 - t1:.3f} s")
    print("hops  roc_auc  avg_prec")
    for hop in range(a.hops):
        roc_auc, avg_prec = res.metrics[hop]
        print(f"{hop:4d}  {roc_auc:.4f}   {avg_prec:.4f}")
    print(f"best: roc_auc {res.test_roc_auc:.4f} at {res.best_hop_roc_auc} hops, avg_prec {res.test_avg_prec:.4f} at {res.best_hop_avg_prec}")


if __name__ == "__main__":
    main()

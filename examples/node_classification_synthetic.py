#!/usr/bin/env python3
"""The node-classification task (NodeClassification: epochs of train + evaluate, then the post-processing step;
sgl/tasks/node_classification.py:11-112, sgl/tasks/utils.py:12-98) on the MI355X, on the device from end to end: the graph is
generated there (a degree-corrected planted partition), the features are planted blobs -- one centre per class under unit noise --
and SGC (K hops of the normalised graph once, then a logistic-regression head) is trained there by `node_classification`: per step
ONE launch for the loss, its gradient and the training accuracy (sgl_class_loss_grad_f32: one read of the logits, one write of
dLogits), per evaluation one arg-max launch per split and one host read for both accuracies.  Run full-batch and, with
--batch, on seeded mini-batches; both with nn.CrossEntropyLoss's arithmetic, or with the reference's LogeCrossEntropy (--loss loge).

    python examples/node_classification_synthetic.py [--nodes 200000] [--edges 2000000] [--classes 8] [--hops 2] [--epochs 20] [--batch 16384]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgl_amd import device as dev, synthetic  # noqa: E402
from sgl_amd.io import DeviceAdjacency  # noqa: E402
from sgl_amd.models.homo import SGC  # noqa: E402
from sgl_amd.tricks import node_classification  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--loss", choices=("cross_entropy", "loge"), default="cross_entropy")
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
    classes = int(y.max()) + 1
    centres = torch.randn((classes, a.dim), generator=g, device=device) * 0.5
    x = dev.alloc_rows(n, a.dim, device)
    x.copy_(centres[y] + torch.randn((n, a.dim), generator=g, device=device))
    order = torch.randperm(n, generator=g, device=device)
    train_idx, val_idx, test_idx = order[:n // 10], order[n // 10:n // 5], order[n // 5:]

    for label, kw in (("full batch", {}), (f"mini-batches of {a.batch}", dict(train_batch_size=a.batch, eval_batch_size=4 * a.batch))):
        torch.manual_seed(a.seed)
        model = SGC(prop_steps=a.hops, feat_dim=a.dim, output_dim=classes)
        torch.cuda.synchronize()
        t0 = time.time()
        res = node_classification(model, adj, x, y, train_idx, val_idx, test_idx, epochs=a.epochs, lr=a.lr, weight_decay=5e-5, loss_fn=a.loss,
                                  seed=a.seed, device=device, **kw)
        torch.cuda.synchronize()
        took = time.time() - t0
        print(f"{label}: {n} nodes, {adj.nnz} stored entries, {classes} classes, {len(train_idx)} training rows, loss {a.loss}: {a.hops} hops + "
              f"{a.epochs} epochs + the post-processing step {took:.3f} s")
        print("epoch  loss      train   val     test")
        for h in res.history:
            loss = f"{h['loss']:8.4f}" if "loss" in h else "        "
            acc = f"{h['acc_train']:.4f}" if "acc_train" in h else "      "
            print(f"{str(h['epoch']):>5}  {loss}  {acc}  {h['acc_val']:.4f}  {h['acc_test']:.4f}")
        print(f"best val {res.best_val:.4f}, its test {res.best_test:.4f}")
        losses = [h["loss"] for h in res.history[:-1]]
        assert all(torch.isfinite(torch.tensor(losses))), losses
        assert res.best_test > 1.5 / classes, "SGC failed to learn the planted classes"


if __name__ == "__main__":
    main()

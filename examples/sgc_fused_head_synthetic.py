#!/usr/bin/env python3
"""SGC with the fused linear head (DESIGN K21): the flow of examples/sgc_synthetic.py, but a training step never forms the [n, C]
logits -- the pre-propagated rows go to tricks.classification.linear_cross_entropy (one launch for the logits on the matrix cores, the
loss, the arg-max and dLogits; two for dW and db), and evaluation is the arg-max-only launch.  The same run without the fused head is
made next to it from the same initial weights.  --in-place adds the run of DESIGN K22, fused_head="in_place": the head reads rows
train_idx of the stored matrix itself (no gathered copy; with --hop-dtype bfloat16 no widened copy either), bit for bit the fused run.

    python examples/sgc_fused_head_synthetic.py [--nodes 19717 --feat 500 --classes 3 --epochs 50 --in-place --hop-dtype bfloat16]"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgc_synthetic import planted_graph  # noqa: E402
from sgl_amd import config  # noqa: E402
from sgl_amd.models.homo import SGC  # noqa: E402
from sgl_amd.tricks import classification as cl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=19717)
    ap.add_argument("--feat", type=int, default=None, help="default 500; 200 with --one-pass")
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--prop-steps", type=int, default=3)
    ap.add_argument("--in-place", action="store_true", help="also run fused_head='in_place' and compare its bits with fused_head=True")
    ap.add_argument("--one-pass", action="store_true",
                    help="also run fused_head='one_pass' and 'one_pass_in_place' (DESIGN K23: loss, dW and db from one read of the rows) and "
                         "compare their weights with fused_head=True; --feat then defaults to 200, inside sgl_linear_step_rule")
    ap.add_argument("--hop-dtype", default="float32", choices=("float32", "bfloat16"))
    a = ap.parse_args()
    a.feat = a.feat or (200 if a.one_pass else 500)
    device = torch.device("cuda")
    config.hop_dtype = a.hop_dtype
    adj, y = planted_graph(a.nodes, a.classes, 5, 0.8, seed=0)
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((a.nodes, a.feat)) + 0.35 * np.eye(a.classes)[y] @ rng.standard_normal((a.classes, a.feat))).astype(np.float32)
    idx = rng.permutation(a.nodes)
    train_idx, val_idx, test_idx = idx[: a.nodes // 5], idx[a.nodes // 5: a.nodes // 2], idx[a.nodes // 2:]
    labels = torch.from_numpy(y).to(device)

    first = SGC(prop_steps=a.prop_steps, feat_dim=a.feat, output_dim=a.classes)
    weights = {}
    for fused in (True, False) + (("in_place",) if a.in_place else ()) + (("one_pass", "one_pass_in_place") if a.one_pass else ()):
        model = copy.deepcopy(first)
        model.preprocess(adj, x)
        model.to(device)
        opt = torch.optim.Adam(model.parameters(), lr=0.1, weight_decay=5e-5)
        for _ in range(a.epochs):
            loss, acc = cl.train(model, train_idx, labels, device, opt, fused_head=fused)
        val, test = cl.evaluate(model, val_idx, test_idx, labels, device, fused_head=fused)
        weights[fused] = model._base_model.linear.weight.detach().clone()
        print(f"fused_head={fused}: epochs {a.epochs}  train loss {loss:.4f}  train acc {acc:.4f}  val acc {val:.4f}  test acc {test:.4f}")
        assert test > 1.5 / a.classes, "SGC failed to learn the planted communities"
    if a.in_place:
        assert torch.equal(weights[True], weights["in_place"]), "the in-place head must give the bits of the fused head"
    if a.one_pass:                                      # another order of the rows in dW: close, not bit-equal
        assert torch.equal(weights["one_pass"], weights["one_pass_in_place"]), "the stored rows must give the bits of the gathered rows"
        gap = float((weights["one_pass"] - weights[True]).abs().max() / weights[True].abs().max())
        print(f"fused_head='one_pass': weights within {gap:.2e} (relative to the largest weight) of fused_head=True")
        assert gap < 1e-2, "the one-pass head drifted from the fused head"


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One training step of link prediction on an edge list: loss and dZ, four ways, on the products shape.

Inputs: N = 2 449 029 random float32 rows (padded buffers), d in --dims; 2^22 positive pairs drawn among the stored entries of the
products-shaped synthetic graph (synthetic.chung_lu_torch with the S1 parameters) and 2^22 uniform negative pairs; labels 1 / 0.
Legs, one step (loss + dZ) each, timed INTERLEAVED in one process (warm-up, then --reps repetitions each, HIP events):
    fused      edge_bce_loss on the EdgePlan: ONE launch of sgl_edge_loss_grad_f32 (+ the fold of cut rows), then g x dZ
    unfused    edge_bce_loss(fused=False), plan reuse without fusing: device.edge_dot, the loss in torch under autograd on E floats,
               one GIVEN-mode launch
    sorted     the path before the plan: edge_scores autograd on a plain edge list -- per step a radix sort into a new CSR, a new SpMM plan
    torch      the torch composition (z[u] * z[v]).sum(1) under autograd (index_add_ backward: float atomics)
and a sweep of max_piece on the fused leg at the first width.  Before anything is timed every leg's loss and sampled gradient rows
are compared with a float64 evaluation of the sampled rows' edges; a mismatch ends the run with a non-zero exit status.

    python tools/bench_edge_loss.py [--reps 20] [--warmup 3] [--dims 100,128] [--pairs 4194304] [--out profiles/edge_loss.json]

Prints one JSON line (and writes it to --out).  No number here is an acceptance criterion."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import device as dev, synthetic  # noqa: E402
from sgl_amd.tricks import EdgePlan, edge_bce_loss, edge_scores  # noqa: E402

PIECES = (128, 256, 512, 1024, 4096, 1 << 40)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return int(peak - base)


def stats(ms):
    a = np.asarray(ms)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def reference_loss_on_logits(s, y):
    """the reference as written: sigmoid, then the with-logits loss (mean)"""
    return F.binary_cross_entropy_with_logits(torch.sigmoid(s), y)


def legs(z, edges, labels, plan):
    u, v = edges[:, 0], edges[:, 1]

    def fused():
        zg = z.detach().requires_grad_(True)
        loss = edge_bce_loss(zg, plan, fused=True)
        loss.backward()
        return loss.detach(), zg.grad

    def unfused():
        zg = z.detach().requires_grad_(True)
        loss = edge_bce_loss(zg, plan, fused=False)
        loss.backward()
        return loss.detach(), zg.grad

    def sorted_():
        zg = z.detach().requires_grad_(True)
        loss = reference_loss_on_logits(edge_scores(zg, edges), labels)
        loss.backward()
        return loss.detach(), zg.grad

    def torch_():
        zg = z.detach().requires_grad_(True)
        loss = reference_loss_on_logits((zg[u] * zg[v]).sum(1), labels)
        loss.backward()
        return loss.detach(), zg.grad

    return {"fused": fused, "unfused": unfused, "sorted": sorted_, "torch": torch_}


def truth_on_sample(z, edges, labels, rows):
    """float64 loss over ALL edges and dZ of the sampled rows, on the device, edge block after edge block"""
    e_total = edges.shape[0]
    loss = torch.zeros((), dtype=torch.float64, device=z.device)
    grad = torch.zeros((rows.numel(), z.shape[1]), dtype=torch.float64, device=z.device)
    slot = torch.full((z.shape[0],), -1, dtype=torch.int64, device=z.device)
    slot[rows] = torch.arange(rows.numel(), device=z.device)
    for lo in range(0, e_total, 1 << 20):
        e = edges[lo:lo + (1 << 20)]
        a, b = z[e[:, 0]].double(), z[e[:, 1]].double()
        s = (a * b).sum(1).requires_grad_(True)
        part = F.binary_cross_entropy_with_logits(torch.sigmoid(s), labels[lo:lo + (1 << 20)].double(), reduction="sum") / e_total
        part.backward()
        loss += part.detach()
        for mine, other in ((e[:, 0], b), (e[:, 1], a)):
            at = slot[mine]
            keep = at >= 0
            grad.index_add_(0, at[keep], s.grad[keep, None] * other[keep])
    return float(loss), grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dims", default="100,128")
    ap.add_argument("--pairs", type=int, default=1 << 22)
    ap.add_argument("--workload", default="S1_products")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_loss.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge_loss.py needs a GPU (nothing here is measured without one)")
    if args.reps < 20:
        print("EXP edge_loss: fewer than 20 repetitions: not a measurement to quote", flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    w = synthetic.WORKLOADS[args.workload]
    n = w["n"]
    rowptr, col, _ = synthetic.chung_lu_torch(n, w["m"], w["d_max"], seed=args.seed, device=device)
    g = torch.Generator(device=device)
    g.manual_seed(args.seed + 11)
    at = torch.randint(0, col.numel(), (args.pairs,), generator=g, device=device)
    rows_of = torch.searchsorted(rowptr, at, right=True) - 1
    pos = torch.stack((rows_of, col[at].to(torch.int64)), dim=1)
    neg = torch.randint(0, n, (args.pairs, 2), generator=g, device=device)
    del rowptr, col, at, rows_of
    edges = torch.cat((pos, neg)).contiguous()
    labels = torch.cat((torch.ones(args.pairs, device=device), torch.zeros(args.pairs, device=device)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    plan = EdgePlan(edges, labels, n, device=device)
    e1.record()
    torch.cuda.synchronize()
    deg = plan.inc_ptr[1:] - plan.inc_ptr[:-1]
    result = {"n": n, "pairs": 2 * args.pairs, "reps": args.reps, "warmup": args.warmup, "plan_build_ms": e0.elapsed_time(e1),
              "max_degree": int(deg.max()), "median_degree": float(deg.double().median()), "pieces_default": plan.n_pieces,
              "partial_rows_default": plan.n_partial, "default_max_piece": plan.max_piece, "dims": {}}
    sample = torch.cat((torch.argsort(deg, descending=True)[:8], torch.randint(0, n, (56,), generator=g, device=device))).unique()
    ok = True
    dims = [int(t) for t in args.dims.split(",")]
    for d in dims:
        z = dev.alloc_rows(n, d, device)
        z.copy_(torch.randn((n, d), generator=g, device=device) * (1.0 / d ** 0.5))
        fns = legs(z, edges, labels, plan)
        want_loss, want_rows = truth_on_sample(z, edges, labels, sample)
        scale = float(want_rows.abs().max())
        entry = {"check": {}, "legs": {}}
        for name, fn in fns.items():
            loss, grad = fn()
            err_l, err_g = abs(float(loss) - want_loss) / want_loss, float((grad[sample].double() - want_rows).abs().max()) / scale
            entry["check"][name] = {"loss_rel_err": err_l, "grad_rows_max_err_over_max": err_g}
            print(f"EXP edge_loss d={d} check {name}: loss rel err {err_l:.2e}, sampled gradient rows max err / max {err_g:.2e}", flush=True)
            ok = ok and err_l < 1e-5 and err_g < 1e-4
            del loss, grad
        if not ok:
            print("EXP edge_loss: a leg disagrees with the float64 evaluation", flush=True)
            raise SystemExit(2)
        peaks = {name: peak_above_inputs(fn) for name, fn in fns.items()}
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(args.reps):                  # interleaved: every leg sees the same drift of the machine
            for name, fn in fns.items():
                ms[name].append(timed(fn))
        # the yardstick from bytes: one edge_dot over the 2 E incidences' worth of row gathers = two edge_dot calls over the list
        dot = stats([timed(lambda: (dev.edge_dot(z, z, plan.edges), dev.edge_dot(z, z, plan.edges))) for _ in range(args.reps)])
        for name in fns:
            entry["legs"][name] = {"ms": stats(ms[name]), "peak_above_inputs_bytes": peaks[name]}
            s = entry["legs"][name]["ms"]
            print(f"EXP edge_loss d={d} {name}: {s['median']:.3f} ms ({s['min']:.3f}-{s['max']:.3f}), peak above inputs "
                  f"{peaks[name] / 2**20:.0f} MiB", flush=True)
        entry["two_edge_dot_ms"] = dot
        print(f"EXP edge_loss d={d} two edge_dot calls over the list: {dot['median']:.3f} ms ({dot['min']:.3f}-{dot['max']:.3f})", flush=True)
        if d == dims[0]:
            plans = {mp: EdgePlan(edges, labels, n, max_piece=mp, device=device) for mp in PIECES}
            sweep = {mp: [] for mp in PIECES}
            runs = {mp: legs(z, edges, labels, p)["fused"] for mp, p in plans.items()}
            for _ in range(args.warmup):
                for fn in runs.values():
                    fn()
            for _ in range(args.reps):
                for mp, fn in runs.items():
                    sweep[mp].append(timed(fn))
            entry["max_piece_sweep"] = {("inf" if mp == PIECES[-1] else str(mp)): dict(stats(sweep[mp]), pieces=plans[mp].n_pieces,
                                                                                      partial_rows=plans[mp].n_partial) for mp in PIECES}
            for k, s in entry["max_piece_sweep"].items():
                print(f"EXP edge_loss d={d} fused, max_piece {k}: {s['median']:.3f} ms ({s['min']:.3f}-{s['max']:.3f}), {s['pieces']} pieces, "
                      f"{s['partial_rows']} partial rows", flush=True)
            del plans, runs
        result["dims"][str(d)] = entry
        del z, fns
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

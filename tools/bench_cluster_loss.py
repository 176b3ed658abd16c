#!/usr/bin/env python3
"""The training step of node clustering: the fused loss-and-gradient kernel (tricks.cluster_loss -> device.
cluster_loss_grad -> sgl_cluster_loss_grad_f32) against the vectorised torch composition a user could write on the device,

    dist = torch.cdist(out, centres); loss = (2 dist.gather(1, y).sum() - dist.mean(1).sum()) / n; loss.backward()

-- the expanded form through a matrix product, an [N, k] matrix kept for the backward, a gradient assembled from several [N, d]
temporaries -- and against the reference's literal expression (sgl/tasks/utils.py:101-113: one torch.norm per centre, torch.cat, and
a Python loop over all rows), which is timed at ONE small n only and quoted per row.

A model output of the S1 row count (N = 2 449 029; random float32 rows around k = 47 centres, contiguous), d in {100, 128, 600}.
Three things are timed per width, INTERLEAVED in one process (warm-up, then --reps repetitions each, HIP events):
  step    cluster_loss(out, y, centres).backward() as autograd runs it (the launch, the float64 row sum, the in-place multiply)
  torch   the composition above, forward and backward
  kernel  the launch alone into preallocated outputs, quoted as a multiple of one read + one write of X at the measured copy
          ceiling (6.29 TB/s)
torch.cuda.max_memory_allocated above the inputs of one step of each is recorded as well.  Before anything is timed, loss and dX of
sampled rows are compared with float64; a mismatch ends the run with a non-zero exit status.

    python tools/bench_cluster_loss.py [--reps 20] [--warmup 3] [--n 2449029] [--k 47] [--out profiles/cluster_loss.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import device as dev, synthetic  # noqa: E402
from sgl_amd.tricks import cluster_loss  # noqa: E402

COPY_CEILING_BYTES_PER_S = 6.29e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


def peak_of(fn):
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


def literal_reference(out, y_pred, centres):
    """the reference's expression as written, Python loop over the rows included"""
    for i in range(len(centres)):
        col = torch.norm(out - centres[i], p=2, dim=1, keepdim=True)
        dist = col if i == 0 else torch.cat((dist, col), 1)
    loss_tmp = -dist.mean(1).sum()
    loss_tmp += 2 * sum(dist[j, x] for j, x in zip(range(dist.shape[0]), y_pred))
    return loss_tmp / dist.shape[0]


def one_width(x, c, y, args):
    n, d = x.shape
    k = c.shape[0]
    w = 1.0 / n
    dx = torch.empty_like(x)
    rows = torch.empty(n, dtype=torch.float32, device=x.device)
    dev.cluster_loss_grad(x, c, y, w, dx=dx, row_loss=rows)
    # values first: sampled rows against float64
    pick = torch.randperm(n, device=x.device)[:4096]
    x64, c64 = x[pick].double().requires_grad_(True), c.double()
    dist = torch.cdist(x64, c64, compute_mode="donot_use_mm_for_euclid_dist")
    per_row = 2 * dist.gather(1, y[pick][:, None])[:, 0] - dist.mean(1)
    (per_row.sum() * w).backward()
    cond = ((2.0 * torch.nn.functional.one_hot(y[pick], k) - 1.0 / k).abs() / dist.detach().clamp_min(1e-300))[:, :, None] \
        * (x64.detach()[:, None, :] - c64[None]).abs()
    err_dx = float(((dx[pick].double() - x64.grad).abs() / (cond.sum(1) * w).clamp_min(1e-300)).max())
    err_rows = float(((rows[pick].double() - per_row.detach()).abs() / (2 * dist.detach().gather(1, y[pick][:, None])[:, 0] + dist.detach().mean(1))).max())
    tol = ((d + 3) / 2 + k + 8) * 2.0 ** -24
    ok = err_dx <= tol and err_rows <= tol
    print(f"EXP cluster_loss d={d}: {len(pick)} sampled rows against float64: worst error of dX {err_dx:.2e} and of the row losses "
          f"{err_rows:.2e}, relative to the sum of the absolute terms (allowed {tol:.2e}){'' if ok else '  WRONG'}", flush=True)
    if not ok:
        raise SystemExit(f"bench_cluster_loss.py: the kernel's values are wrong at d={d}; nothing was timed")
    del x64, c64, dist, per_row, cond
    out = x.detach().requires_grad_(True)

    def kernel():
        return dev.cluster_loss_grad(x, c, y, w, dx=dx, row_loss=rows)

    def step():
        out.grad = None
        loss = cluster_loss(out, y, c, check=False)
        loss.backward()
        return loss

    def step_torch():
        out.grad = None
        dist = torch.cdist(out, c)
        loss = (2 * dist.gather(1, y[:, None]).sum() - dist.mean(1).sum()) / n
        loss.backward()
        return loss

    a, b = float(step().detach()), float(step_torch().detach())
    print(f"EXP cluster_loss d={d}: loss {a:.6f} (kernel step) / {b:.6f} (torch composition)", flush=True)
    peak_k, peak_t = peak_of(step), peak_of(step_torch)
    for _ in range(args.warmup):
        step()
        step_torch()
        kernel()
    torch.cuda.synchronize()
    ms = {"step": [], "torch": [], "kernel": []}
    for _ in range(args.reps):                     # interleaved: all candidates see the same drift of the machine
        ms["step"].append(timed(step))
        ms["torch"].append(timed(step_torch))
        ms["kernel"].append(timed(kernel))
    s = {key: stats(v) for key, v in ms.items()}
    spread = max(v["max"] - v["min"] for v in (s["step"], s["torch"]))
    read_write_ms = 2.0 * n * d * 4 / COPY_CEILING_BYTES_PER_S * 1e3
    r = {"step_ms": s["step"], "torch_ms": s["torch"], "kernel_ms": s["kernel"], "ratio_step_over_torch": s["step"]["median"] / s["torch"]["median"],
         "spread_ms": spread, "step_peak_above_inputs_bytes": peak_k, "torch_peak_above_inputs_bytes": peak_t,
         "read_plus_write_of_x_ms": read_write_ms, "kernel_over_read_plus_write_of_x": s["kernel"]["median"] / read_write_ms,
         "kernel_tflops": 7.0 * n * k * d / (s["kernel"]["median"] * 1e-3) * 1e-12,   # per element and centre: 2 x (subtract), square-add (2), scale-add (2), ~1
         "faster": "kernel" if s["step"]["median"] <= s["torch"]["median"] else "torch"}
    print(f"EXP cluster_loss d={d}: step {s['step']['median']:.3f} ms ({s['step']['min']:.3f}-{s['step']['max']:.3f}), torch composition "
          f"{s['torch']['median']:.3f} ms ({s['torch']['min']:.3f}-{s['torch']['max']:.3f}), ratio {r['ratio_step_over_torch']:.3f}; kernel alone "
          f"{s['kernel']['median']:.3f} ms = {r['kernel_over_read_plus_write_of_x']:.2f} x one read + one write of X at the copy ceiling "
          f"({read_write_ms:.3f} ms); temporaries {peak_k / 2**20:.0f} against {peak_t / 2**20:.0f} MiB", flush=True)
    return r


def literal_cost(args, device, g):
    """the reference's literal expression at one small n: ms per step and microseconds per row (its Python loop is linear in n)"""
    n, d, k = args.literal_n, 100, args.k
    c = torch.randn((k, d), generator=g, device=device)
    x = torch.randn((n, d), generator=g, device=device) + c[torch.randint(0, k, (n,), generator=g, device=device)]
    y = torch.cdist(x, c).argmin(1).cpu().numpy()
    out = x.requires_grad_(True)
    times = []
    for _ in range(3):
        out.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        literal_reference(out, y, c).backward()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    ms = float(np.median(times))
    print(f"EXP cluster_loss: the reference's literal expression at n={n}, d={d}, k={k}: {ms:.1f} ms per step = {ms * 1e3 / n:.1f} us per row "
          f"(not run at the full shape)", flush=True)
    return {"n": n, "d": d, "k": k, "ms": ms, "us_per_row": ms * 1e3 / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=synthetic.WORKLOADS["S1_products"]["n"])
    ap.add_argument("--k", type=int, default=47)
    ap.add_argument("--dims", default="100,128,600")
    ap.add_argument("--literal-n", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_loss.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster_loss.py needs a GPU (nothing here is measured without one)")
    if args.reps < 20:
        print("EXP cluster_loss: fewer than 20 repetitions: not a measurement to quote", flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    g = torch.Generator(device=device)
    g.manual_seed(args.seed)
    result = {"n_rows": args.n, "k": args.k, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(device),
              "copy_ceiling_bytes_per_s": COPY_CEILING_BYTES_PER_S, "shapes": {}}
    result["literal_reference"] = literal_cost(args, device, g)
    for d in [int(v) for v in args.dims.split(",")]:
        c = torch.randn((args.k, d), generator=g, device=device, dtype=torch.float32)
        x = torch.randn((args.n, d), generator=g, device=device, dtype=torch.float32)
        x += c[torch.randint(0, args.k, (args.n,), generator=g, device=device)]
        y = dev.kmeans_assign(x, c, want_dist=False)[0]
        result["shapes"][f"d{d}"] = {"d": d, **one_width(x, c, y, args)}
        del x, c, y
        torch.cuda.empty_cache()
    result["kernel_slower_at"] = [key for key, v in result["shapes"].items() if v["faster"] != "kernel"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP cluster_loss wrote {args.out}", flush=True)
    print("EXP cluster_loss " + ("the fused step is the faster one at every width" if not result["kernel_slower_at"]
                                 else f"the torch composition is faster at {result['kernel_slower_at']}"), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The fused linear head (DESIGN K21) against the torch head it replaces, on one MI355X.

    python tools/bench_head.py [--reps 20 --warmup 3 --out profiles/linear_head.json]

Shapes: N = 2 449 029 (all nodes) and 196 615 (the products train split), (d, C) = (100, 47), (128, 172), (500, 3).  Every leg's two
candidates are interleaved in one process, 3 warm-ups + 20 repetitions, HIP events, median (min - max):
  (a) forward + loss + dZ: device.linear_class_loss against F.linear + device.class_loss_grad (K14);
  (b) a whole step with dW and db: linear_cross_entropy + backward against cross_entropy(F.linear(...)) + backward (torch autograd);
  (c) evaluation: the arg-max-only launch against F.linear + predict;
  (d) one read of X at the copy ceiling, the yardstick.
Before timing, the fused outputs of 64 sampled rows are checked against float64 inside the header's bounds.  The comparison point is the
torch path of the same process; nothing is compared against itself."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import _lib, device as dev  # noqa: E402
from sgl_amd.tricks import classification as cl  # noqa: E402

COPY_CEILING_BYTES_PER_S = 6.29e12
SHAPES = ((100, 47), (128, 172), (500, 3))
ROWS = (2449029, 196615)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


def stats(ms):
    a = np.asarray(ms)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def compare(fused, torch_path, args, tag):
    for _ in range(args.warmup):
        fused()
        torch_path()
    torch.cuda.synchronize()
    ms_f, ms_t = [], []
    for _ in range(args.reps):                     # interleaved: both candidates see the same drift of the machine
        ms_f.append(timed(fused))
        ms_t.append(timed(torch_path))
    sf, st = stats(ms_f), stats(ms_t)
    r = {"fused_ms": sf, "torch_ms": st, "ratio_fused_over_torch": sf["median"] / st["median"],
         "expectation_lower_time": "confirmed" if sf["max"] < st["min"] else ("refuted" if sf["min"] > st["max"] else "undecided")}
    print(f"EXP head {tag}: fused {sf['median']:.3f} ms ({sf['min']:.3f}-{sf['max']:.3f}), torch {st['median']:.3f} ms "
          f"({st['min']:.3f}-{st['max']:.3f}), ratio {r['ratio_fused_over_torch']:.3f} {r['expectation_lower_time']}", flush=True)
    return r


def check_sample(x, w, b, y, dz, loss, pred):
    """64 sampled rows against float64 inside the header's bounds; raises on a miss"""
    rows = torch.linspace(0, x.shape[0] - 1, 64, device=x.device).long()
    d, c = x.shape[1], w.shape[0]
    x64, w64 = x[rows].double().cpu().numpy(), w.double().cpu().numpy()
    z = x64 @ w64.T + b.double().cpu().numpy()
    e = ((d + 3) * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T + np.abs(b.cpu().numpy()))).max(1)
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    p, yy = np.exp(z - lse[:, None]), y[rows].cpu().numpy()
    want = lse - z[np.arange(64), yy]
    onehot = np.zeros_like(z)
    onehot[np.arange(64), yy] = 1
    assert (np.abs(loss[rows].cpu().numpy() - want) <= 2 * e + (c + 16) * 2.0 ** -23 + 2.0 ** -23 * (np.abs(lse) + np.abs(want))).all()
    tol = p * (np.expm1(2 * e)[:, None] + (c + 8 + np.abs(z - m[:, None])) * 2.0 ** -23) + 2.0 ** -23
    assert (np.abs(dz[rows].cpu().numpy() - (p - onehot)) <= tol).all()
    assert (z[np.arange(64), pred[rows].cpu().numpy()] >= m - 2 * e).all()


def one_shape(n, d, c, args):
    dev_ = torch.device("cuda", 0)
    gen = torch.Generator(device=dev_).manual_seed(args.seed)
    x = dev.alloc_rows(n, d, dev_)
    x.copy_(torch.randn((n, d), generator=gen, device=dev_))
    lin = torch.nn.Linear(d, c).to(dev_)
    w, b = lin.weight, lin.bias
    y = torch.randint(0, c, (n,), generator=gen, device=dev_)
    dz_buf, z_buf = dev.alloc_rows(n, c, dev_), dev.alloc_rows(n, c, dev_)
    wd, bd = w.detach(), b.detach()
    dz, loss, pred, _ = dev.linear_class_loss(x, wd, bd, y, 1.0, dz=dz_buf, row_loss=True, pred=True)
    check_sample(x, wd, bd, y, dz, loss, pred)
    out = {"n": n, "d": d, "c": c}

    def torch_fwd():
        z = torch.addmm(bd, x, wd.t(), out=z_buf) if z_buf.is_contiguous() else F.linear(x, wd, bd)
        return dev.class_loss_grad(z, y, 1.0, dz=dz_buf, row_loss=True, pred=True)

    out["a_forward_loss_dz"] = compare(lambda: dev.linear_class_loss(x, wd, bd, y, 1.0, dz=dz_buf, row_loss=True, pred=True), torch_fwd, args,
                                       f"(a) n={n} d={d} C={c}")

    def step(fused):
        lin.zero_grad(set_to_none=True)
        loss_ = cl.linear_cross_entropy(x, w, b, y, check=False) if fused else cl.cross_entropy(F.linear(x, w, b), y, check=False)
        loss_.backward()
        return loss_

    out["b_whole_step"] = compare(lambda: step(True), lambda: step(False), args, f"(b) n={n} d={d} C={c}")
    out["c_evaluation"] = compare(lambda: dev.linear_class_loss(x, wd, bd, None, 1.0, pred=True), lambda: cl.predict(F.linear(x, wd, bd)), args,
                                  f"(c) n={n} d={d} C={c}")
    out["d_one_read_of_x_ms"] = n * d * 4 / COPY_CEILING_BYTES_PER_S * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_head.json"))
    args = ap.parse_args()
    _lib.require_gpu()
    torch.cuda.set_device(0)
    results = [one_shape(int(n), d, c, args) for n in args.rows.split(",") for d, c in SHAPES]
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "copy_ceiling_bytes_per_s": COPY_CEILING_BYTES_PER_S,
           "protocol": "legs interleaved in one process, HIP events, median (min - max); fused outputs of 64 sampled rows checked against float64 first",
           "not_measured": ["hardware counters (LDS bank conflicts, FETCH bytes)", "mini-batch steps below 196 615 rows", "C > 172"],
           "results": results}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

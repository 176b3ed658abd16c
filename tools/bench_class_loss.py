#!/usr/bin/env python3
"""The loss part of a node-classification step: the fused loss / gradient / arg-max kernel (tricks.cross_entropy ->
device.class_loss_grad -> sgl_class_loss_grad_f32) against the torch composition a user writes on the device today,

    loss = F.cross_entropy(out, y); loss.backward(); correct = out.max(1)[1].eq(y).sum()

-- a log-softmax forward, the NLL gather, an arg-max, the NLL backward and the log-softmax backward over [B, C] logits.

Shapes: the training rows and all nodes of the products workload with its 47 classes (B = 196 615, N = 2 449 029), N rows of the 172
classes of papers100M, and the pubmed training shape (B = 19 717, C = 3); random float32 logits, contiguous.  Per shape these legs are
timed INTERLEAVED in one process (warm-up, then --reps repetitions each, HIP events around work that ends in a synchronise):
  step     (a) cross_entropy(out, y, check=False, fused=True, return_pred=True), backward, and the correct count
  torch    (b) the composition above
  again    (a) and (b) once more each, timed as legs of their own: the spread between two runs of the SAME leg, which a difference
           between (a) and (b) has to exceed to count
  kernel   (c) the launch alone into preallocated outputs, quoted as a multiple of one read + one write of the logits at the measured
           copy ceiling (6.29 TB/s)
  pred     (d) predict(out) against out.max(1)[1]
torch.cuda.max_memory_allocated above the inputs of one step of each is recorded as well.  Before anything is timed, loss, dLogits and
the arg-max of sampled rows are compared with float64; a mismatch ends the run with a non-zero exit status.

    python tools/bench_class_loss.py [--reps 20] [--warmup 3] [--out profiles/class_loss.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import device as dev  # noqa: E402
from sgl_amd.tricks import cross_entropy, predict  # noqa: E402

COPY_CEILING_BYTES_PER_S = 6.29e12
SHAPES = (("products_train", 196_615, 47), ("products_all", 2_449_029, 47), ("papers_classes", 2_449_029, 172), ("pubmed_train", 19_717, 3))
DECIDING = ("products_train", "products_all")      # the default of fused=None is decided at the two C = 47 shapes


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


def check_values(z, y, name):
    """sampled rows against float64: the row losses, dLogits (w = 1) and the arg-max"""
    n, c = z.shape
    dz, rows, pred = dev.class_loss_grad(z, y, 1.0, dz=True, row_loss=True, pred=True)
    pick = torch.randperm(n, device=z.device)[:4096]
    z64 = z[pick].double().requires_grad_(True)
    per_row = F.cross_entropy(z64, y[pick], reduction="none")
    per_row.sum().backward()
    lse = torch.logsumexp(z64.detach(), 1)
    # (the sum of the exponentials is at least 1 and carries up to c roundings: log s is off by up to c 2^-24 ABSOLUTE, whatever |lse| is)
    err_rows = float(((rows[pick].double() - per_row.detach()).abs() / (lse.abs() + z64.detach().gather(1, y[pick][:, None])[:, 0].abs() + 1.0)).max())
    err_dz = float((dz[pick].double() - z64.grad).abs().max())       # (a probability or a probability minus one: absolute)
    same_pred = bool((pred[pick] == z[pick].max(1)[1]).all())
    tol = (c + 16) * 2.0 ** -24
    ok = err_rows <= tol and err_dz <= tol and same_pred
    print(f"EXP class_loss {name}: {len(pick)} sampled rows against float64: worst error of the row losses {err_rows:.2e} (relative to "
          f"|lse| + |z_y| + 1) and of dZ {err_dz:.2e} (allowed {tol:.2e}), arg-max {'equal' if same_pred else 'DIFFERENT'}{'' if ok else '  WRONG'}",
          flush=True)
    if not ok:
        raise SystemExit(f"bench_class_loss.py: the kernel's values are wrong at {name}; nothing was timed")


def one_shape(name, n, c, args, g, device):
    z = torch.randn((n, c), generator=g, device=device, dtype=torch.float32) * 3.0
    y = torch.randint(0, c, (n,), generator=g, device=device)
    check_values(z, y, name)
    w = 1.0 / n
    dz = torch.empty_like(z)
    rows = torch.empty(n, dtype=torch.float32, device=device)
    pred = torch.empty(n, dtype=torch.int64, device=device)
    out = z.detach().requires_grad_(True)

    def kernel():
        return dev.class_loss_grad(z, y, w, dz=dz, row_loss=rows, pred=pred)

    def step():
        out.grad = None
        loss, p = cross_entropy(out, y, check=False, fused=True, return_pred=True)
        loss.backward()
        return loss, p.eq(y).sum()

    def step_torch():
        out.grad = None
        loss = F.cross_entropy(out, y)
        loss.backward()
        return loss, out.detach().max(1)[1].eq(y).sum()

    def pred_ours():
        return predict(z)

    def pred_torch():
        return z.max(1)[1]

    (a, ca), (b, cb) = step(), step_torch()
    print(f"EXP class_loss {name}: loss {float(a.detach()):.6f} (kernel step) / {float(b.detach()):.6f} (torch composition), correct "
          f"{int(ca)} / {int(cb)}", flush=True)
    peaks = {key: peak_of(fn) for key, fn in (("step", step), ("torch", step_torch), ("pred", pred_ours), ("pred_torch", pred_torch))}
    legs = {"step": step, "torch": step_torch, "step_again": step, "torch_again": step_torch, "kernel": kernel, "pred": pred_ours,
            "pred_torch": pred_torch}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {key: [] for key in legs}
    for _ in range(args.reps):                     # interleaved: all candidates see the same drift of the machine
        for key, fn in legs.items():
            ms[key].append(timed(fn))
    s = {key: stats(v) for key, v in ms.items()}
    spread = max(abs(s["step"]["median"] - s["step_again"]["median"]), abs(s["torch"]["median"] - s["torch_again"]["median"]))
    read_write_ms = 2.0 * n * c * 4 / COPY_CEILING_BYTES_PER_S * 1e3
    gap = s["torch"]["median"] - s["step"]["median"]
    r = {"n": n, "c": c, "step_ms": s["step"], "torch_ms": s["torch"], "step_again_ms": s["step_again"], "torch_again_ms": s["torch_again"],
         "kernel_ms": s["kernel"], "pred_ms": s["pred"], "pred_torch_ms": s["pred_torch"],
         "ratio_step_over_torch": s["step"]["median"] / s["torch"]["median"], "ratio_pred_over_torch": s["pred"]["median"] / s["pred_torch"]["median"],
         "spread_between_runs_of_one_leg_ms": spread, "peak_above_inputs_bytes": peaks,
         "read_plus_write_of_logits_ms": read_write_ms, "kernel_over_read_plus_write_of_logits": s["kernel"]["median"] / read_write_ms,
         "pred_over_one_read_of_logits": s["pred"]["median"] / (read_write_ms / 2),
         "faster": "kernel" if gap > spread else ("torch" if -gap > spread else "neither")}
    print(f"EXP class_loss {name} (n={n}, c={c}): step {s['step']['median']:.3f} ms ({s['step']['min']:.3f}-{s['step']['max']:.3f}), torch "
          f"composition {s['torch']['median']:.3f} ms ({s['torch']['min']:.3f}-{s['torch']['max']:.3f}), ratio {r['ratio_step_over_torch']:.3f}, "
          f"spread between two runs of one leg {spread:.3f} ms; kernel alone {s['kernel']['median']:.3f} ms = "
          f"{r['kernel_over_read_plus_write_of_logits']:.2f} x one read + one write of the logits at the copy ceiling ({read_write_ms:.3f} ms); "
          f"pred {s['pred']['median']:.3f} ms ({s['pred']['min']:.3f}-{s['pred']['max']:.3f}) against max(1)[1] {s['pred_torch']['median']:.3f} ms "
          f"({s['pred_torch']['min']:.3f}-{s['pred_torch']['max']:.3f}); temporaries {peaks['step'] / 2**20:.1f} against "
          f"{peaks['torch'] / 2**20:.1f} MiB (step), {peaks['pred'] / 2**20:.1f} against {peaks['pred_torch'] / 2**20:.1f} MiB (pred)", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_loss.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_class_loss.py needs a GPU (nothing here is measured without one)")
    if args.reps < 20:
        print("EXP class_loss: fewer than 20 repetitions: not a measurement to quote", flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    g = torch.Generator(device=device)
    g.manual_seed(args.seed)
    result = {"reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(device),
              "copy_ceiling_bytes_per_s": COPY_CEILING_BYTES_PER_S, "shapes": {}}
    wanted = args.shapes.split(",")
    for name, n, c in SHAPES:
        if name in wanted:
            result["shapes"][name] = one_shape(name, n, c, args, g, device)
            torch.cuda.empty_cache()
    verdicts = [result["shapes"][k]["faster"] for k in DECIDING if k in result["shapes"]]
    result["verdict"] = ("not measured" if len(verdicts) < len(DECIDING) else "kernel" if all(v == "kernel" for v in verdicts)
                         else "torch" if all(v == "torch" for v in verdicts) else "undecided")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP class_loss wrote {args.out}", flush=True)
    print(f"EXP class_loss verdict at {DECIDING}: {result['verdict']} (per shape: {verdicts})", flush=True)


if __name__ == "__main__":
    main()

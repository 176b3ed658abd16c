#!/usr/bin/env python3
"""The aggregator part of a NARS training step: one forward plus backward of the sub-graph ensemble aggregator alone,
the fused path (models.simple_models.*OneDimConvolution.combine -> device.ensemble_combine -> sgl_ensemble_combine_f32 /
sgl_ensemble_combine_bwd_f32) against the reference's torch formulation on the same device,

    per_feature   out_h = (stack([x[idx] for x in X[h]], dim=2) * W[h].unsqueeze(0)).mean(dim=2)         sgl/models/simple_models.py:22-31
    fast          out   = (T[idx] @ W).squeeze(2),  T the [N, d, S * H] tensor stacked once at preprocess   simple_models.py:78-79

followed by sum_h <out_h, G_h>.backward() for the weight gradient.

Shape: S = 8 sub-graphs, K = 3 (H = 4 hops), B = 50 000 rows out of N = 736 389 (the ogbn-mag paper count), d = 128 and 256; random
float32 matrices on the line-aware pitch, a random index with repeats.  Per (mode, d) the legs are timed INTERLEAVED in one process
(warm-up, then --reps repetitions each, HIP events around work that ends in a synchronise):
  fused / torch   the two formulations
  again           each once more, as legs of their own: the spread between two runs of the SAME leg, which a difference has to exceed
  forward only    the fused forward alone (no_grad), quoted against its algorithmic bytes -- (M + H) B d 4 -- at the measured copy
                  ceiling (6.29 TB/s)
Before anything is timed, outputs and weight gradients of the two are compared (and a sample of output rows with float64); a mismatch
ends the run with a non-zero exit status.

    python tools/bench_ensemble.py [--reps 20] [--warmup 3] [--out profiles/ensemble_combine.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import device as dev  # noqa: E402
from sgl_amd.models import simple_models as sm  # noqa: E402

COPY_CEILING_BYTES_PER_S = 6.29e12
N_ROWS, BATCH, S, H = 736_389, 50_000, 8, 4
WIDTHS = (128, 256)


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


def torch_step(mode, X, T, params, idx, G):
    for p in params:
        p.grad = None
    if mode == "fast":
        outs = [(T[idx] @ params[0]).squeeze(dim=2)]
    else:
        outs = [(torch.stack([x[idx] for x in X[h]], dim=2) * params[h].unsqueeze(dim=0)).mean(dim=2) for h in range(H)]
    sum((o * g).sum() for o, g in zip(outs, G)).backward()
    return outs, [p.grad for p in params]


def fused_step(mod, X, idx, G):
    mod.zero_grad(set_to_none=True)
    outs = mod.combine(X, idx)
    outs = outs if isinstance(outs, list) else [outs]
    sum((o * g).sum() for o, g in zip(outs, G)).backward()
    return outs, [p.grad for p in mod.parameters()]


def run(mode, d, reps, warmup, cuda):
    gen = torch.Generator(device=cuda)
    gen.manual_seed(1000 + d)
    X = [[dev.alloc_rows(N_ROWS, d, cuda) for _ in range(S)] for _ in range(H)]
    for row in X:
        for x in row:
            x.normal_(generator=gen)
    idx = torch.randint(0, N_ROWS, (BATCH,), device=cuda, generator=gen)
    n_out = 1 if mode == "fast" else H
    G = [torch.randn((BATCH, d), device=cuda, generator=gen) for _ in range(n_out)]
    mod = (sm.FastOneDimConvolution(S, H) if mode == "fast" else sm.OneDimConvolution(S, H, d)).to(cuda)
    with torch.no_grad():
        for p in mod.parameters():
            p.uniform_(0.5, 1.5, generator=gen)
    params = [p.detach().clone().requires_grad_() for p in mod.parameters()]
    # the reference's own input of the fast form: stacked once, outside the step
    T = torch.stack([torch.stack(X[h], dim=2) for h in range(H)], dim=3).view(N_ROWS, d, S * H) if mode == "fast" else None

    fo, fg = fused_step(mod, X, idx, G)
    to, tg = torch_step(mode, X, T, params, idx, G)
    worst_o = max(float((a.detach() - b.detach()).abs().max() / b.detach().abs().max()) for a, b in zip(fo, to))
    worst_g = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fg, tg))
    pick = torch.arange(0, BATCH, 97, device=cuda)
    if mode == "fast":
        want = sum(X[h][s][idx[pick]].double() * params[0][s * H + h, 0].double() for s in range(S) for h in range(H))
    else:
        want = sum(X[0][s][idx[pick]].double() * params[0][:, s].double()[None, :] for s in range(S)) / S
    worst_64 = float((fo[0].detach()[pick].double() - want.detach()).abs().max() / want.detach().abs().max())
    ok = worst_o < 1e-5 and worst_g < 1e-4 and worst_64 < 1e-6
    print(f"{mode} d={d}: fused vs torch: outputs {worst_o:.2e}, weight gradients {worst_g:.2e}; fused vs float64 (sampled rows) {worst_64:.2e}"
          f"  {'ok' if ok else 'MISMATCH'}", flush=True)
    if not ok:
        raise SystemExit(1)
    del fo, fg, to, tg

    def forward_only():
        with torch.no_grad():
            return mod.combine(X, idx)

    legs = {"fused": lambda: fused_step(mod, X, idx, G), "torch": lambda: torch_step(mode, X, T, params, idx, G),
            "fused_again": lambda: fused_step(mod, X, idx, G), "torch_again": lambda: torch_step(mode, X, T, params, idx, G),
            "fused_forward": forward_only}
    ms = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            t = timed(fn)
            if r >= warmup:
                ms[k].append(t)
    m_total = S * H
    fwd_bytes = (m_total + n_out) * BATCH * d * 4
    res = {"mode": mode, "d": d, "S": S, "H": H, "B": BATCH, "N": N_ROWS, "legs_ms": {k: stats(v) for k, v in ms.items()},
           "forward_algorithmic_bytes": fwd_bytes, "torch_forward_bytes_estimate": (7 * m_total + n_out) * BATCH * d * 4,
           "check": {"outputs_vs_torch": worst_o, "grads_vs_torch": worst_g, "outputs_vs_float64": worst_64}}
    fwd = res["legs_ms"]["fused_forward"]["median"] * 1e-3
    res["forward_fraction_of_copy_ceiling"] = fwd_bytes / fwd / COPY_CEILING_BYTES_PER_S
    res["step_speedup_median"] = res["legs_ms"]["torch"]["median"] / res["legs_ms"]["fused"]["median"]
    res["same_leg_spread"] = max(abs(res["legs_ms"][k]["median"] / res["legs_ms"][k + "_again"]["median"] - 1.0) for k in ("fused", "torch"))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_combine.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cuda = torch.device("cuda", 0)
    results = []
    for d in WIDTHS:
        for mode in ("per_feature", "fast"):
            results.append(run(mode, d, a.reps, a.warmup, cuda))
            torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "copy_ceiling_bytes_per_s": COPY_CEILING_BYTES_PER_S, "reps": a.reps, "warmup": a.warmup,
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

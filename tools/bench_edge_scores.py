#!/usr/bin/env python3
"""Edge scores of link prediction: the direct kernel (device.edge_dot -> sgl_edge_dot_f32) against the torch
expression a user had to write before it, `(z[u] * z[v]).sum(1)` -- three passes and two [E, d] temporaries.

A feature matrix of the S1 row count (N = 2 449 029; random float32 rows in a row_pitch(d) buffer), d in {100, 128, 600},
E = 2^22 pairs, drawn (a) uniformly and (b) from the S1 benchmark graph's own edges (synthetic.chung_lu_torch with the S1
parameters: the degree-skewed pairs a link-prediction task scores).  Both candidates run INTERLEAVED in one process (warm-up, then
--reps repetitions each, HIP events); torch.cuda.max_memory_allocated of one call of each is recorded as well.  Before anything is
timed, sampled scores of the kernel are compared with a float64 evaluation; a mismatch ends the run with a non-zero exit status.

    python tools/bench_edge_scores.py [--reps 20] [--warmup 3] [--n 2449029] [--edges 4194304] [--out profiles/edge_scores.json]

Per shape and edge source the JSON holds: ms of both candidates (median, min, max), their ratio, the fraction of 8 TB/s the kernel
reaches by algorithmic bytes E (2 d 4 + 16 + 4), and the peak allocation of both.  "accepted": the kernel's median is below the
torch expression's."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import device as dev, synthetic  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


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
    return int(peak), int(peak - base)


def stats(ms):
    a = np.asarray(ms)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def graph_pairs(n, n_edges, seed, device):
    """n_edges stored non-zeros (row, column) of the S1-law graph over n nodes, drawn uniformly among its non-zeros"""
    w = synthetic.WORKLOADS["S1_products"]
    m = int(w["m"] * (n / w["n"]))
    rowptr, col, _ = synthetic.chung_lu_torch(n, m, w["d_max"], seed=seed, device=device)
    g = torch.Generator(device=device)
    g.manual_seed(seed + 7)
    at = torch.randint(0, int(col.numel()), (n_edges,), generator=g, device=device)
    u = torch.searchsorted(rowptr, at, right=True) - 1
    return torch.stack((u, col[at].to(torch.int64)), dim=1).contiguous()


def one_case(z, edges, args, tag):
    n, d = z.shape
    n_e = edges.shape[0]
    u, v = edges[:, 0].contiguous(), edges[:, 1].contiguous()

    def kernel():
        return dev.edge_dot(z, z, edges)

    def expression():
        return (z[u] * z[v]).sum(1)

    # values first: sampled scores against float64
    got = kernel()
    pick = torch.randperm(n_e, device=z.device)[:4096]
    zu, zv = z[u[pick]].double(), z[v[pick]].double()
    truth, cond = (zu * zv).sum(1), (zu.abs() * zv.abs()).sum(1)
    worst = float(((got[pick].double() - truth).abs() / cond.clamp_min(1e-30)).max())
    ok = worst <= 1e-5 and bool(torch.isfinite(got).all())
    print(f"EXP edge_scores {tag}: {len(pick)} sampled scores against float64: worst |err| / sum|terms| = {worst:.2e}"
          f"{'' if ok else '  WRONG'}", flush=True)
    if not ok:
        raise SystemExit(f"bench_edge_scores.py: the kernel's scores are wrong at {tag}; nothing was timed")
    del got, zu, zv, truth, cond
    peak_k, extra_k = peak_of(kernel)
    peak_t, extra_t = peak_of(expression)
    for _ in range(args.warmup):
        kernel()
        expression()
    torch.cuda.synchronize()
    ms_k, ms_t = [], []
    for _ in range(args.reps):                     # interleaved: both candidates see the same drift of the machine
        ms_k.append(timed(kernel))
        ms_t.append(timed(expression))
    sk, st = stats(ms_k), stats(ms_t)
    algo = n_e * (2 * d * 4 + 16 + 4)
    r = {"kernel_ms": sk, "torch_ms": st, "ratio_kernel_over_torch": sk["median"] / st["median"], "algorithmic_bytes": int(algo),
         "kernel_fraction_of_8TBps": algo / (sk["median"] * 1e-3) / PEAK_BYTES_PER_S, "kernel_peak_bytes": peak_k,
         "torch_peak_bytes": peak_t, "kernel_peak_above_inputs_bytes": extra_k, "torch_peak_above_inputs_bytes": extra_t,
         "distinct_rows_touched": int(torch.unique(edges).numel())}
    r["accepted"] = bool(sk["median"] < st["median"])
    print(f"EXP edge_scores {tag}: kernel {sk['median']:.3f} ms ({sk['min']:.3f}-{sk['max']:.3f}), torch {st['median']:.3f} ms "
          f"({st['min']:.3f}-{st['max']:.3f}), ratio {r['ratio_kernel_over_torch']:.3f}, {r['kernel_fraction_of_8TBps']:.3f} of 8 TB/s, "
          f"peak above inputs {extra_k / 2**20:.0f} against {extra_t / 2**20:.0f} MiB{'' if r['accepted'] else '  NOT ACCEPTED'}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=synthetic.WORKLOADS["S1_products"]["n"])
    ap.add_argument("--edges", type=int, default=1 << 22)
    ap.add_argument("--dims", default="100,128,600")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_scores.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge_scores.py needs a GPU (nothing here is measured without one)")
    if args.reps < 20:
        print("EXP edge_scores: fewer than 20 repetitions: not a measurement to quote", flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    g = torch.Generator(device=device)
    g.manual_seed(args.seed)
    sources = {"uniform": torch.randint(0, args.n, (args.edges, 2), generator=g, device=device),
               "graph": graph_pairs(args.n, args.edges, args.seed, device)}
    torch.cuda.empty_cache()
    result = {"n_rows": args.n, "n_edges": args.edges, "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(device), "peak_bytes_per_s": PEAK_BYTES_PER_S, "shapes": {}}
    failed = []
    for d in [int(v) for v in args.dims.split(",")]:
        z = dev.alloc_rows(args.n, d, device)
        z.copy_(torch.randn((args.n, d), generator=g, device=device, dtype=torch.float32))
        for name, edges in sources.items():
            r = one_case(z, edges, args, f"d={d} {name}")
            result["shapes"][f"d{d}_{name}"] = {"d": d, "pitch": int(z.stride(0)), "edges": name, **r}
            if not r["accepted"]:
                failed.append(f"d{d}_{name}")
        del z
        torch.cuda.empty_cache()
    result["not_accepted"] = failed
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP edge_scores wrote {args.out}", flush=True)
    print("EXP edge_scores " + ("every shape accepted" if not failed else f"NOT ACCEPTED: {failed}"), flush=True)


if __name__ == "__main__":
    main()

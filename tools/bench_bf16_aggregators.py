#!/usr/bin/env python3
"""The full-matrix aggregators over bfloat16 hops: reading the stored hops in place (sgl_hop_reduce_bf16_f32,
sgl_hop_concat_bf16 / _f32, sgl_nafs_bf16_f32) against the route they replace, which stays callable: device.widen_hops (every hop
copied into a float32 matrix of its own) followed by the float32 entry.

Hop matrices of the S1 row count (N = 2 449 029; random bfloat16 values in row_pitch(d, 2) buffers, no graph needed), d in
{100, 128, 147} x H in {4, 11}, for mean, concat (bfloat16 and float32 result) and NAFS.  Both routes run INTERLEAVED in one
process (warm-up, then --reps repetitions each, HIP events); torch.cuda.max_memory_allocated of one call of each route is recorded
as well.  Before anything is timed, sampled rows of each direct result are compared with the widening route's bit for bit; a
mismatch ends the run with a non-zero exit status.  If the device cannot hold a shape at N rows, N is halved for that shape and
the JSON says so.

    python tools/bench_bf16_aggregators.py [--reps 20] [--warmup 3] [--n 2449029] [--out profiles/bf16_aggregators.json]

Per shape and aggregator the JSON holds: ms of both routes (median, min, max), their ratio, the fraction of 8 TB/s the direct route
reaches by algorithmic bytes (H n d 2 + n d_out (2 or 4)), and the peak allocation of both.  "accepted": the direct route's median
is not above the widening route's and its peak allocation is below it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import _lib, device as dev, synthetic  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def make_hops(n, d, H, device, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    hops = []
    for h in range(H):
        t = dev.alloc_rows(n, d, device, dtype=torch.bfloat16)
        t.copy_(torch.randn((n, d), generator=g, device=device, dtype=torch.float32) * (1.0 - 0.04 * h))
        hops.append(t)
    return hops


def routes(kind, hops):
    """(direct, widening): callables that return the aggregate"""
    if kind == "mean":
        return (lambda: dev.hop_reduce(_lib.SGL_REDUCE_MEAN, hops)), (lambda: dev.hop_reduce(_lib.SGL_REDUCE_MEAN, dev.widen_hops(hops)))
    if kind == "concat_bf16":
        return (lambda: dev.hop_concat(hops, out_dtype=torch.bfloat16)), (lambda: dev.hop_concat(dev.widen_hops(hops)))
    if kind == "concat_f32":
        return (lambda: dev.hop_concat(hops)), (lambda: dev.hop_concat(dev.widen_hops(hops)))
    return (lambda: dev.nafs_aggregate(hops)), (lambda: dev.nafs_aggregate(dev.widen_hops(hops)))


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


def one_shape(n, d, H, args, device, rows):
    hops = make_hops(n, d, H, device, seed=args.seed + 100 * d + H)
    res = {}
    for kind in ("mean", "concat_bf16", "concat_f32", "nafs"):
        direct, widening = routes(kind, hops)
        # values first: sampled rows of the direct result against the widening route's, bit for bit
        a, b = direct(), widening()
        idx = torch.from_numpy(rows[rows < n]).to(device)
        ga, gb = a[idx].float().cpu().numpy(), b[idx].cpu().numpy()
        same = ga.shape == gb.shape and np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
        print(f"EXP bf16_agg d={d} H={H} {kind}: {len(idx)} sampled rows against the widening route: {'bit-equal' if same else 'DIFFER'}",
              flush=True)
        if not same:
            raise SystemExit(f"bench_bf16_aggregators.py: {kind} at d={d}, H={H} does not return the widening route's bits; nothing was timed")
        d_out = a.shape[1]
        out_bytes = a.element_size()
        del a, b, ga, gb
        peak_d, extra_d = peak_of(direct)
        peak_w, extra_w = peak_of(widening)
        for _ in range(args.warmup):
            direct()
            widening()
        torch.cuda.synchronize()
        ms_d, ms_w = [], []
        for _ in range(args.reps):                 # interleaved: both routes see the same drift of the machine
            ms_d.append(timed(direct))
            ms_w.append(timed(widening))
        sd, sw = stats(ms_d), stats(ms_w)
        algo = H * n * d * 2 + n * d_out * out_bytes
        r = {"direct_ms": sd, "widening_ms": sw, "ratio_direct_over_widening": sd["median"] / sw["median"],
             "algorithmic_bytes": int(algo), "direct_fraction_of_8TBps": algo / (sd["median"] * 1e-3) / PEAK_BYTES_PER_S,
             "direct_peak_bytes": peak_d, "widening_peak_bytes": peak_w, "direct_peak_above_hops_bytes": extra_d,
             "widening_peak_above_hops_bytes": extra_w, "result_dtype": "bfloat16" if out_bytes == 2 else "float32", "result_columns": int(d_out)}
        r["accepted"] = bool(sd["median"] <= sw["median"] and peak_d < peak_w)
        res[kind] = r
        print(f"EXP bf16_agg d={d} H={H} {kind}: direct {sd['median']:.3f} ms ({sd['min']:.3f}-{sd['max']:.3f}), widening "
              f"{sw['median']:.3f} ms ({sw['min']:.3f}-{sw['max']:.3f}), ratio {r['ratio_direct_over_widening']:.3f}, "
              f"{r['direct_fraction_of_8TBps']:.3f} of 8 TB/s, peak {peak_d / 2**30:.2f} against {peak_w / 2**30:.2f} GiB"
              f"{'' if r['accepted'] else '  NOT ACCEPTED'}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=synthetic.WORKLOADS["S1_products"]["n"])
    ap.add_argument("--dims", default="100,128,147")
    ap.add_argument("--hops", default="4,11")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_aggregators.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bf16_aggregators.py needs a GPU (nothing here is measured without one)")
    if args.reps < 20:
        print("EXP bf16_agg: fewer than 20 repetitions: not a measurement to quote", flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    rows = np.unique(np.concatenate([np.random.default_rng(args.seed).integers(0, args.n, 4096), [0, args.n - 1]])).astype(np.int64)
    result = {"n_rows_requested": args.n, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(device),
              "peak_bytes_per_s": PEAK_BYTES_PER_S, "shapes": {}}
    failed = []
    for d in [int(v) for v in args.dims.split(",")]:
        for H in [int(v) for v in args.hops.split(",")]:
            n = args.n
            while True:
                try:
                    res = one_shape(n, d, H, args, device, rows)
                    break
                except torch.cuda.OutOfMemoryError:
                    torch.cuda.empty_cache()
                    n //= 2
                    print(f"EXP bf16_agg d={d} H={H}: out of memory, retrying with n = {n}", flush=True)
                    if n < 1024:
                        raise
            result["shapes"][f"d{d}_H{H}"] = {"n_rows": n, "d": d, "n_hops": H, "hop_pitch_elements": dev.row_pitch(d, elem_size=2), **res}
            failed += [f"d{d}_H{H}:{k}" for k, v in res.items() if not v["accepted"]]
            torch.cuda.empty_cache()
    result["not_accepted"] = failed
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP bf16_agg wrote {args.out}", flush=True)
    print("EXP bf16_agg " + ("every shape accepted" if not failed else f"NOT ACCEPTED: {failed}"), flush=True)


if __name__ == "__main__":
    main()

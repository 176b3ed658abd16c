#!/usr/bin/env python3
"""The k-means step of node clustering: the assignment kernel (device.kmeans_assign -> sgl_kmeans_assign_f32) against
the torch composition a user had to write before it, `torch.cdist(x, c).argmin(1)` -- the expanded form through a matrix product,
an [N, k] matrix written and read again -- and one whole Lloyd iteration (assignment + the membership-matrix SpMM of
tricks/clustering.py) against that composition plus `index_add_` (floating-point atomics) and `bincount`.

A feature matrix of the S1 row count (N = 2 449 029; random float32 rows around k = 47 centres, contiguous), d in {100, 128, 600}.
Both candidates run INTERLEAVED in one process (warm-up, then --reps repetitions each, HIP events); torch.cuda.max_memory_allocated
of one call of each is recorded as well.  Before anything is timed, the labels of sampled rows are compared with a float64 argmin; a
mismatch ends the run with a non-zero exit status.

    python tools/bench_kmeans.py [--reps 20] [--warmup 3] [--n 2449029] [--k 47] [--out profiles/kmeans.json]

Per width the JSON holds: ms of both candidates (median, min, max) for the assignment and for the iteration, their ratios, the
assignment as a multiple of ONE read of X at the measured copy ceiling (6.29 TB/s), and the peak allocation of both.
"accepted": the kernel's median is not above the composition's by more than the spread (max - min) the repetitions of the two
recorded."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import device as dev, synthetic  # noqa: E402
from sgl_amd.tricks import clustering  # noqa: E402

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


def compare(ours, theirs, args, tag):
    extra_o, extra_t = peak_of(ours), peak_of(theirs)
    for _ in range(args.warmup):
        ours()
        theirs()
    torch.cuda.synchronize()
    ms_o, ms_t = [], []
    for _ in range(args.reps):                     # interleaved: both candidates see the same drift of the machine
        ms_o.append(timed(ours))
        ms_t.append(timed(theirs))
    so, st = stats(ms_o), stats(ms_t)
    spread = max(so["max"] - so["min"], st["max"] - st["min"])
    r = {"kernel_ms": so, "torch_ms": st, "ratio_kernel_over_torch": so["median"] / st["median"], "spread_ms": spread,
         "kernel_peak_above_inputs_bytes": extra_o, "torch_peak_above_inputs_bytes": extra_t,
         "accepted": bool(so["median"] <= st["median"] + spread)}
    print(f"EXP kmeans {tag}: ours {so['median']:.3f} ms ({so['min']:.3f}-{so['max']:.3f}), torch {st['median']:.3f} ms "
          f"({st['min']:.3f}-{st['max']:.3f}), ratio {r['ratio_kernel_over_torch']:.3f}, temporaries {extra_o / 2**20:.0f} against "
          f"{extra_t / 2**20:.0f} MiB{'' if r['accepted'] else '  NOT ACCEPTED'}", flush=True)
    return r


def one_width(x, c, args):
    n, d = x.shape
    k = c.shape[0]
    # values first: the labels of sampled rows against a float64 argmin (rows near a tie may go either way: count them apart)
    labels, mindist = dev.kmeans_assign(x, c)
    pick = torch.randperm(n, device=x.device)[:4096]
    dist = torch.cdist(x[pick].double(), c.double()) ** 2
    two = torch.topk(dist, 2, dim=1, largest=False).values
    clear = (two[:, 1] - two[:, 0]) > (d + 3) * 2.0 ** -22 * two[:, 1]
    wrong = int(((labels[pick] != dist.argmin(1)) & clear).sum())
    worst = float(((mindist[pick].double() - two[:, 0]).abs() / two[:, 0].clamp_min(1e-300)).max())
    ok = wrong == 0 and worst <= (d + 3) * 2.0 ** -23
    print(f"EXP kmeans d={d}: {len(pick)} sampled rows against float64: {wrong} wrong labels away from ties, worst relative "
          f"distance error {worst:.2e}{'' if ok else '  WRONG'}", flush=True)
    if not ok:
        raise SystemExit(f"bench_kmeans.py: the kernel's labels are wrong at d={d}; nothing was timed")
    del labels, mindist, dist, two
    update = clustering._Update(x, k)

    def assign():
        return dev.kmeans_assign(x, c)

    def assign_torch():
        return torch.cdist(x, c).argmin(1)

    def iteration():
        lab, md = dev.kmeans_assign(x, c)
        return update(lab, md)

    def iteration_torch():
        lab = torch.cdist(x, c).argmin(1)
        sums = torch.zeros((k, d), dtype=torch.float32, device=x.device).index_add_(0, lab, x)
        return sums / torch.bincount(lab, minlength=k).to(torch.float32)[:, None]

    r = {"assign": compare(assign, assign_torch, args, f"d={d} assign"),
         "iteration": compare(iteration, iteration_torch, args, f"d={d} Lloyd iteration")}
    one_read_ms = n * d * 4 / COPY_CEILING_BYTES_PER_S * 1e3
    r["one_read_of_x_ms"] = one_read_ms
    r["assign_over_one_read_of_x"] = r["assign"]["kernel_ms"]["median"] / one_read_ms
    r["assign_gflop"] = 2.0 * n * k * d * 1e-9
    r["assign_tflops"] = 3.0 * n * k * d / (r["assign"]["kernel_ms"]["median"] * 1e-3) * 1e-12      # subtract, multiply, add
    print(f"EXP kmeans d={d}: assignment = {r['assign_over_one_read_of_x']:.2f} x one read of X at the copy ceiling "
          f"({one_read_ms:.3f} ms), {r['assign_tflops']:.1f} TFLOP/s", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=synthetic.WORKLOADS["S1_products"]["n"])
    ap.add_argument("--k", type=int, default=47)
    ap.add_argument("--dims", default="100,128,600")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans.py needs a GPU (nothing here is measured without one)")
    if args.reps < 20:
        print("EXP kmeans: fewer than 20 repetitions: not a measurement to quote", flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    g = torch.Generator(device=device)
    g.manual_seed(args.seed)
    result = {"n_rows": args.n, "k": args.k, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(device),
              "copy_ceiling_bytes_per_s": COPY_CEILING_BYTES_PER_S, "shapes": {}}
    failed = []
    for d in [int(v) for v in args.dims.split(",")]:
        c = torch.randn((args.k, d), generator=g, device=device, dtype=torch.float32)
        x = torch.randn((args.n, d), generator=g, device=device, dtype=torch.float32)
        x += c[torch.randint(0, args.k, (args.n,), generator=g, device=device)]
        c = x[torch.randint(0, args.n, (args.k,), generator=g, device=device)].clone()       # a seeding, not the optimum
        r = one_width(x, c, args)
        result["shapes"][f"d{d}"] = {"d": d, **r}
        failed += [f"d{d}_{what}" for what in ("assign", "iteration") if not r[what]["accepted"]]
        del x, c
        torch.cuda.empty_cache()
    result["not_accepted"] = failed
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP kmeans wrote {args.out}", flush=True)
    print("EXP kmeans " + ("every shape accepted" if not failed else f"NOT ACCEPTED: {failed}"), flush=True)


if __name__ == "__main__":
    main()

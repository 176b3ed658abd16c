#!/usr/bin/env python3
"""The k-means step of node clustering: the assignment kernel (device.kmeans_assign -> sgl_kmeans_assign_f32) against
the torch composition a user had to write before it, `torch.cdist(x, c).argmin(1)` -- the expanded form through a matrix product,
an [N, k] matrix written and read again -- and one whole Lloyd iteration (assignment + the membership-matrix SpMM of
tricks/clustering.py) against that composition plus `index_add_` (floating-point atomics) and `bincount`.

A feature matrix of the S1 row count (N = 2 449 029; random float32 rows around k = 47 centres, contiguous), d in {100, 128, 600}.
Both candidates run INTERLEAVED in one process (warm-up, then --reps repetitions each, HIP events); torch.cuda.max_memory_allocated
of one call of each is recorded as well.  Before anything is timed, the labels of sampled rows are compared with a float64 argmin; a
mismatch ends the run with a non-zero exit status.

    python tools/bench_kmeans.py [--reps 20] [--warmup 3] [--n 2449029] [--k 47] [--out profiles/kmeans.json] [--seed-only]

Per width the JSON holds: ms of both candidates (median, min, max) for the assignment and for the iteration, their ratios, the
assignment as a multiple of ONE read of X at the measured copy ceiling (6.29 TB/s), and the peak allocation of both.
"accepted": the kernel's median is not above the composition's by more than the spread (max - min) the repetitions of the two
recorded.

The matrix leg (--matrix-out, default profiles/kmeans_matrix.json; --matrix-only skips the two-way legs above): the
matrix-core form (form="matrix"), the direct kernel and the torch composition interleaved THREE ways under the same protocol, labels
of sampled rows checked against float64 first (the bound of include/sgl_kmeans_mfma.h), one Lloyd iteration per form, and
"matrix_faster": the matrix form's min-max lies wholly below the direct kernel's.

The sums leg (--sums-out, default profiles/kmeans_sums.json; --sums-only runs nothing else): the centre update alone in
both forms -- the membership-matrix SpMM (update="spmm") and the one-pass kernel (device.cluster_sums, update="sums") -- and the whole
iteration, matrix assignment + update, in both forms, the four interleaved under the same protocol.  Both updates are checked against
float64 sums of sampled clusters first.  "sums_faster": the new update's min-max lies wholly below the SpMM update's.

The seeding leg (--seed-out, default profiles/kmeans_seed.json; --seed-only runs nothing else): one whole seeding of k
centres by the torch k-means++ of tricks/clustering.py (_seed_plus_plus), by the step kernel with one candidate per step
(device.kmeans_seed, trials=1) and with five, interleaved under the same protocol, draws uploaded inside the timed call as kmeans
does.  First the kernel's `near` must equal, bit for bit, the assignment kernel's minimum over the centres it chose, and its last
potential their float64 sum.  Then one kmeans call of --seed-n-init runs under each init, Lloyd loop capped at --seed-max-iter
iterations (matrix assignment, one-pass sums), timed once with a host clock.  "trials1_below_torch": the min-max of trials=1 lies
wholly below the torch seeding's; "trials5_not_above_torch": the median of trials=5 is not above the torch seeding's."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import _lib, device as dev, synthetic  # noqa: E402
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


def matrix_leg(x, c, args):
    """matrix form, direct kernel and torch.cdist().argmin interleaved in one process; one Lloyd iteration per form"""
    n, d = x.shape
    k = c.shape[0]
    shift = c.mean(0)
    labels, mindist = dev.kmeans_assign(x, c, form="matrix")
    pick = torch.randperm(n, device=x.device)[:4096]
    dist = torch.stack([((x[pick].double() - cj.double()) ** 2).sum(1) for cj in c], dim=1)      # differences first: exact zeros stay zeros
    xn, cn = (x[pick].double() - shift.double()).norm(dim=1)[:, None], (c.double() - shift.double()).norm(dim=1)[None, :]
    bound = (d + 3) * 2.0 ** -23 * (cn ** 2 + 2 * xn * cn) + 2.0 ** -23 * dist.sqrt() * (xn + cn)
    got, best = labels[pick][:, None], dist.argmin(1)[:, None]
    excess = (dist.gather(1, got) - dist.gather(1, best)) - 2 * (bound.gather(1, got) + bound.gather(1, best))
    worst = float(((mindist[pick].double() - dist.gather(1, got)[:, 0]).abs() / dist.gather(1, got)[:, 0].clamp_min(1e-300)).max())
    differ = int((got != best).sum())
    ok = float(excess.max()) <= 0 and worst <= (d + 3) * 2.0 ** -23
    print(f"EXP kmeans-matrix d={d}: {len(pick)} sampled rows against float64: {differ} labels off the argmin, largest excess over the "
          f"bound {float(excess.max()):.3e}, worst relative distance error {worst:.2e}{'' if ok else '  WRONG'}", flush=True)
    if not ok:
        raise SystemExit(f"bench_kmeans.py: the matrix form's labels are wrong at d={d}; nothing was timed")
    del labels, mindist, dist, bound, excess
    update = clustering._Update(x, k)
    legs = {"matrix": lambda: dev.kmeans_assign(x, c, form="matrix"), "matrix_labels_only": lambda: dev.kmeans_assign(x, c, want_dist=False, form="matrix"),
            "direct": lambda: dev.kmeans_assign(x, c), "torch": lambda: torch.cdist(x, c).argmin(1),
            "iteration_matrix": lambda: update(*dev.kmeans_assign(x, c, form="matrix")), "iteration_direct": lambda: update(*dev.kmeans_assign(x, c))}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.reps):                     # interleaved: every candidate sees the same drift of the machine
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    r = {name + "_ms": stats(v) for name, v in ms.items()}
    one_read_ms = n * d * 4 / COPY_CEILING_BYTES_PER_S * 1e3
    r["one_read_of_x_ms"] = one_read_ms
    for name in ("matrix", "matrix_labels_only", "direct"):
        r[name + "_over_one_read_of_x"] = r[name + "_ms"]["median"] / one_read_ms
    r["matrix_tflops"] = 2.0 * n * k * d / (r["matrix_ms"]["median"] * 1e-3) * 1e-12
    r["matrix_faster"] = bool(r["matrix_ms"]["max"] < r["direct_ms"]["min"])
    print(f"EXP kmeans-matrix d={d}: " + ", ".join(f"{name} {r[name + '_ms']['median']:.3f} ms ({r[name + '_ms']['min']:.3f}-{r[name + '_ms']['max']:.3f})"
                                                  for name in legs) + f"; matrix = {r['matrix_over_one_read_of_x']:.2f} x one read of X "
          f"({one_read_ms:.3f} ms), {'faster than' if r['matrix_faster'] else 'NOT wholly below'} the direct kernel", flush=True)
    return r


def sums_leg(x, c, args):
    """the centre update in both forms, alone and behind the matrix assignment, interleaved in one process"""
    n, d = x.shape
    k = c.shape[0]
    labels, mindist = dev.kmeans_assign(x, c, form="matrix")
    old, new = clustering._Update(x, k), clustering._Update(x, k, "sums")
    (s_old, n_old), (s_new, n_new) = old.sums(labels), new.sums(labels)
    rule = (ctypes.c_int64 * 5)()
    _lib.check(_lib.lib().sgl_cluster_sums_rule(n, d, k, 1, rule), "sgl_cluster_sums_rule")
    worst = {"spmm": 0.0, "sums": 0.0}
    ok = bool(torch.equal(n_old, n_new))
    for j in torch.randperm(k)[:8].tolist():       # sampled clusters against float64; the bound of include/sgl_cluster_sums.h
        rows = x[labels == j].double()
        exact, mass = rows.sum(0), rows.abs().sum(0).clamp_min(1e-300)
        ok = ok and int(n_new[j]) == rows.shape[0]
        for name, got in (("spmm", s_old), ("sums", s_new)):
            worst[name] = max(worst[name], float(((got[j].double() - exact).abs() / mass).max()))
    bound = (rule[0] + rule[1]) * 2.0 ** -24
    ok = ok and worst["sums"] <= bound
    print(f"EXP kmeans-sums d={d}: B={rule[0]} R={rule[1]} slab={rule[2]} S={rule[3]} LDS={rule[4]} B; 8 sampled clusters against float64, error / sum|x|: "
          f"spmm {worst['spmm']:.2e}, sums {worst['sums']:.2e} (bound {bound:.2e}){'' if ok else '  WRONG'}", flush=True)
    if not ok:
        raise SystemExit(f"bench_kmeans.py: the one-pass sums are wrong at d={d}; nothing was timed")
    del s_old, s_new, rows
    legs = {"update_spmm": lambda: old(labels, mindist), "update_sums": lambda: new(labels, mindist),
            "iteration_spmm": lambda: old(*dev.kmeans_assign(x, c, form="matrix")), "iteration_sums": lambda: new(*dev.kmeans_assign(x, c, form="matrix"))}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.reps):                     # interleaved: every candidate sees the same drift of the machine
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    r = {name + "_ms": stats(v) for name, v in ms.items()}
    one_read_ms = n * d * 4 / COPY_CEILING_BYTES_PER_S * 1e3
    r.update(one_read_of_x_ms=one_read_ms, blocks=rule[0], rows_per_block=rule[1], slab=rule[2], slabs=rule[3], lds_bytes=rule[4],
             error_over_sum_abs=worst, error_bound=bound)
    for name in ("update_spmm", "update_sums"):
        r[name + "_over_one_read_of_x"] = r[name + "_ms"]["median"] / one_read_ms
    r["sums_faster"] = bool(r["update_sums_ms"]["max"] < r["update_spmm_ms"]["min"])
    r["iteration_faster"] = bool(r["iteration_sums_ms"]["max"] < r["iteration_spmm_ms"]["min"])
    print(f"EXP kmeans-sums d={d}: " + ", ".join(f"{name} {r[name + '_ms']['median']:.3f} ms ({r[name + '_ms']['min']:.3f}-{r[name + '_ms']['max']:.3f})"
                                                for name in legs) + f"; update_sums = {r['update_sums_over_one_read_of_x']:.2f} x one read of X "
          f"({one_read_ms:.3f} ms), {'wholly below' if r['sums_faster'] else 'NOT wholly below'} the SpMM update", flush=True)
    return r


def seed_leg(x, args):
    """one whole seeding: the torch k-means++, the step kernel with 1 and with 5 candidates per step; a kmeans call under each init"""
    import time
    n, d = x.shape
    k = args.k
    rule = (ctypes.c_int64 * 5)()
    _lib.check(_lib.lib().sgl_kmeans_seed_rule(n, d, 5, rule), "sgl_kmeans_seed_rule")
    gen = torch.Generator().manual_seed(args.seed)
    same = {}
    for trials in (1, 5):                          # values first: near against the assignment kernel over the chosen centres
        ids, near, pot = dev.kmeans_seed(x, k, torch.rand((k, trials), generator=gen, dtype=torch.float64).to(x.device), trials)
        want = dev.kmeans_assign(x, x[ids])[1]
        total = float(want.sum(dtype=torch.float64))
        ok = bool(torch.equal(near.view(torch.int32), want.view(torch.int32))) and abs(float(pot[-1]) - total) <= 1e-9 * total
        same[trials] = int(torch.unique(ids).numel())
        print(f"EXP kmeans-seed d={d} trials={trials}: {same[trials]} distinct centres of {k}, near {'equals' if ok else 'DIFFERS FROM'} the "
              f"assignment kernel's minimum, last potential {float(pot[-1]):.6e} against {total:.6e}{'' if ok else '  WRONG'}", flush=True)
        if not ok:
            raise SystemExit(f"bench_kmeans.py: the seeding kernel's distances are wrong at d={d}; nothing was timed")
    del ids, near, pot, want
    legs = {"torch": lambda: clustering._seed_plus_plus(x, k, gen), "trials1": lambda: clustering._seed_greedy(x, k, gen, 1),
            "trials5": lambda: clustering._seed_greedy(x, k, gen, 5)}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.reps):                     # interleaved: every candidate sees the same drift of the machine
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    r = {name + "_ms": stats(v) for name, v in ms.items()}
    one_read_ms = n * d * 4 / COPY_CEILING_BYTES_PER_S * 1e3
    r.update(one_read_of_x_ms=one_read_ms, steps=k, blocks=rule[0], rows_per_block=rule[1], lds_bytes_trials5=rule[4], distinct_centres=same)
    for name in legs:
        r[name + "_step_over_one_read_of_x"] = r[name + "_ms"]["median"] / k / one_read_ms
    r["trials1_below_torch"] = bool(r["trials1_ms"]["max"] < r["torch_ms"]["min"])
    r["trials5_not_above_torch"] = bool(r["trials5_ms"]["median"] <= r["torch_ms"]["median"])
    print(f"EXP kmeans-seed d={d}: " + ", ".join(f"{name} {r[name + '_ms']['median']:.3f} ms ({r[name + '_ms']['min']:.3f}-{r[name + '_ms']['max']:.3f}), "
                                                f"{r[name + '_step_over_one_read_of_x']:.2f} x one read of X per step" for name in legs)
          + f" (one read {one_read_ms:.3f} ms); trials=1 {'wholly below' if r['trials1_below_torch'] else 'NOT wholly below'} the torch seeding, trials=5 "
          f"{'not above' if r['trials5_not_above_torch'] else 'ABOVE'} it", flush=True)
    r["kmeans_call"] = {"n_init": args.seed_n_init, "max_iter": args.seed_max_iter, "assign": "matrix", "update": "sums", "timed": "once, host clock"}
    for init in clustering.KMEANS_INITS:           # what a user calls; the Lloyd loop is the same code under both
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run = clustering.kmeans(x, k, n_init=args.seed_n_init, max_iter=args.seed_max_iter, seed=args.seed, init=init, assign="matrix", update="sums")
        torch.cuda.synchronize()
        r["kmeans_call"][init] = {"seconds": time.perf_counter() - t0, "inertia": run.inertia, "n_iter": run.n_iter}
        print(f"EXP kmeans-seed d={d}: kmeans(n_init={args.seed_n_init}, max_iter={args.seed_max_iter}, init={init!r}): "
              f"{r['kmeans_call'][init]['seconds']:.2f} s, inertia {run.inertia:.6e}", flush=True)
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
    ap.add_argument("--matrix-out", default=os.path.join(ROOT, "profiles", "kmeans_matrix.json"))
    ap.add_argument("--matrix-only", action="store_true")
    ap.add_argument("--sums-out", default=os.path.join(ROOT, "profiles", "kmeans_sums.json"))
    ap.add_argument("--sums-only", action="store_true")
    ap.add_argument("--seed-out", default=os.path.join(ROOT, "profiles", "kmeans_seed.json"))
    ap.add_argument("--seed-only", action="store_true")
    ap.add_argument("--seed-n-init", type=int, default=20)
    ap.add_argument("--seed-max-iter", type=int, default=20)
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
    matrix = {key: result[key] for key in ("n_rows", "k", "reps", "warmup", "device", "copy_ceiling_bytes_per_s")}
    matrix["shapes"] = {}
    sums = dict(matrix, shapes={})
    seeding = dict(matrix, shapes={})
    for d in [int(v) for v in args.dims.split(",")]:
        c = torch.randn((args.k, d), generator=g, device=device, dtype=torch.float32)
        x = torch.randn((args.n, d), generator=g, device=device, dtype=torch.float32)
        x += c[torch.randint(0, args.k, (args.n,), generator=g, device=device)]
        c = x[torch.randint(0, args.n, (args.k,), generator=g, device=device)].clone()       # a seeding, not the optimum
        if not (args.matrix_only or args.sums_only):
            seeding["shapes"][f"d{d}"] = {"d": d, **seed_leg(x, args)}
        if not (args.matrix_only or args.seed_only):
            sums["shapes"][f"d{d}"] = {"d": d, **sums_leg(x, c, args)}
        if not (args.sums_only or args.seed_only):
            matrix["shapes"][f"d{d}"] = {"d": d, **matrix_leg(x, c, args)}
        if not (args.matrix_only or args.sums_only or args.seed_only):
            r = one_width(x, c, args)
            result["shapes"][f"d{d}"] = {"d": d, **r}
            failed += [f"d{d}_{what}" for what in ("assign", "iteration") if not r[what]["accepted"]]
        del x, c
        torch.cuda.empty_cache()
    result["not_accepted"] = failed
    if args.seed_out and not (args.matrix_only or args.sums_only):
        os.makedirs(os.path.dirname(os.path.abspath(args.seed_out)), exist_ok=True)
        with open(args.seed_out, "w") as f:
            json.dump(seeding, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP kmeans wrote {args.seed_out}", flush=True)
    if args.sums_out and not (args.matrix_only or args.seed_only):
        os.makedirs(os.path.dirname(os.path.abspath(args.sums_out)), exist_ok=True)
        with open(args.sums_out, "w") as f:
            json.dump(sums, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP kmeans wrote {args.sums_out}", flush=True)
    if args.matrix_out and not (args.sums_only or args.seed_only):
        os.makedirs(os.path.dirname(os.path.abspath(args.matrix_out)), exist_ok=True)
        with open(args.matrix_out, "w") as f:
            json.dump(matrix, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP kmeans wrote {args.matrix_out}", flush=True)
    if args.out and not (args.matrix_only or args.sums_only or args.seed_only):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP kmeans wrote {args.out}", flush=True)
    print("EXP kmeans " + ("every shape accepted" if not failed else f"NOT ACCEPTED: {failed}"), flush=True)


if __name__ == "__main__":
    main()

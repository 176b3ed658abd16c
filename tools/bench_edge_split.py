#!/usr/bin/env python3
"""The edge split of link prediction: the row-local search kernels (device.csr_find -> sgl_csr_find,
device.edge_candidates -> sgl_edge_candidates) and the whole tricks.mask_test_edges, against the torch formulation a user had before
them: ONE global sorted key array row * n + col (int64, 8 bytes per stored entry, built once and kept) and torch.searchsorted in it.

The graph is the products-shaped synthetic one (synthetic.chung_lu_torch with the S1 parameters: N = 2 449 029, 2 x 61.9 M stored
entries).  Timed, INTERLEAVED in one process (warm-up, then --reps repetitions each, HIP events):
    find_stored   2^26 pairs drawn among the stored entries             kernel / searchsorted
    find_random   2^26 uniform pairs (almost all absent)                kernel / searchsorted
    candidates    2^26 candidates of the stream with their keys         kernel / torch.randint pairs + searchsorted + the key expression
    split         the whole mask_test_edges(seed)                       as shipped / with the torch candidates in place of the kernel
Before anything is timed the kernel's answers are compared with the torch formulation's on every pair of both lists; a mismatch ends
the run with a non-zero exit status.  The torch candidates use torch.randint, not the hash: the same work, other pairs.

    python tools/bench_edge_split.py [--reps 20] [--warmup 3] [--pairs 67108864] [--workload S1_products] [--out profiles/edge_split.json]

Prints one JSON line (and writes it to --out): ms of both sides (median, min, max), their ratio, the bytes of the key array and the
time to build it, the peak allocation of one call of each.  No number here is an acceptance criterion."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import device as dev, synthetic  # noqa: E402
from sgl_amd.io import DeviceAdjacency  # noqa: E402
from sgl_amd.tricks import link_prediction as lp  # noqa: E402


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


def global_keys(adj):
    """the torch formulation's index: row * n_cols + col of every stored entry -- sorted as it stands for a canonical CSR"""
    rows = torch.repeat_interleave(torch.arange(adj.shape[0], dtype=torch.int64, device=adj.device), adj.rowptr[1:] - adj.rowptr[:-1])
    return rows * adj.shape[1] + adj.col


def torch_find(keys, n_cols, edges):
    want = edges[:, 0] * n_cols + edges[:, 1]
    at = torch.searchsorted(keys, want).clamp_(max=keys.numel() - 1)
    return torch.where(keys[at] == want, at, -1)


def torch_candidates(keys, n, count, generator):
    edges = torch.randint(0, n, (count, 2), generator=generator, device=keys.device)
    i, j = edges[:, 0], edges[:, 1]
    stored = torch_find(keys, n, edges) >= 0
    key = torch.where((i != j) & ~stored, torch.minimum(i, j) * n + torch.maximum(i, j), -1)
    return edges, key


def compare(name, kernel, expression, args, result):
    extra_k, extra_t = peak_above_inputs(kernel), peak_above_inputs(expression)
    for _ in range(args.warmup):
        kernel()
        expression()
    torch.cuda.synchronize()
    ms_k, ms_t = [], []
    for _ in range(args.reps):                      # interleaved: both sides see the same drift of the machine
        ms_k.append(timed(kernel))
        ms_t.append(timed(expression))
    sk, st = stats(ms_k), stats(ms_t)
    result[name] = {"kernel_ms": sk, "torch_ms": st, "ratio_kernel_over_torch": sk["median"] / st["median"],
                    "kernel_peak_above_inputs_bytes": extra_k, "torch_peak_above_inputs_bytes": extra_t}
    print(f"EXP edge_split {name}: kernel {sk['median']:.3f} ms ({sk['min']:.3f}-{sk['max']:.3f}), torch {st['median']:.3f} ms "
          f"({st['min']:.3f}-{st['max']:.3f}), ratio {sk['median'] / st['median']:.3f}, peak above inputs {extra_k / 2**20:.0f} against "
          f"{extra_t / 2**20:.0f} MiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1 << 26)
    ap.add_argument("--workload", default="S1_products")
    ap.add_argument("--split-reps", type=int, default=10, help="repetitions of the whole split (each allocates about 10 GiB)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_split.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge_split.py needs a GPU (nothing here is measured without one)")
    if args.reps < 20:
        print("EXP edge_split: fewer than 20 repetitions: not a measurement to quote", flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    w = synthetic.WORKLOADS[args.workload]
    n = w["n"]
    adj = DeviceAdjacency(*synthetic.chung_lu_torch(n, w["m"], w["d_max"], seed=args.seed, device=device), (n, n))
    g = torch.Generator(device=device)
    g.manual_seed(args.seed + 7)
    at = torch.randint(0, adj.nnz, (args.pairs,), generator=g, device=device)
    stored = torch.stack((torch.searchsorted(adj.rowptr, at, right=True) - 1, adj.col[at].to(torch.int64)), dim=1).contiguous()
    uniform = torch.randint(0, n, (args.pairs, 2), generator=g, device=device)
    del at
    result = {"workload": args.workload, "n": n, "nnz": adj.nnz, "pairs": args.pairs, "reps": args.reps, "warmup": args.warmup,
              "split_reps": args.split_reps, "device": torch.cuda.get_device_name(device)}

    result["key_array_build_ms"] = stats([timed(lambda: global_keys(adj)) for _ in range(3)])
    keys = global_keys(adj)
    assert bool((keys[1:] > keys[:-1]).all())
    result["key_array_bytes"] = int(keys.numel() * keys.element_size())
    print(f"EXP edge_split {args.workload}: n = {n}, nnz = {adj.nnz}, key array {result['key_array_bytes'] / 2**20:.0f} MiB, built in "
          f"{result['key_array_build_ms']['median']:.1f} ms", flush=True)

    # values first: every pair of both lists, and the candidates' verdicts, against the torch formulation
    for name, edges, least in (("stored", stored, args.pairs), ("uniform", uniform, 0)):
        got, want = dev.csr_find(adj, edges), torch_find(keys, n, edges)
        if not torch.equal(got, want) or int((got >= 0).sum()) < least:
            raise SystemExit(f"bench_edge_split.py: sgl_csr_find disagrees with searchsorted on the {name} pairs; nothing was timed")
        del got, want
    edges, key = dev.edge_candidates(adj, args.seed, 0, args.pairs)
    i, j = edges[:, 0], edges[:, 1]
    want = torch.where((i != j) & (torch_find(keys, n, edges) < 0), torch.minimum(i, j) * n + torch.maximum(i, j), -1)
    if not torch.equal(key, want):
        raise SystemExit("bench_edge_split.py: sgl_edge_candidates' keys disagree with searchsorted; nothing was timed")
    result["candidates_refused_fraction"] = float((key < 0).double().mean())
    del edges, key, i, j, want
    print("EXP edge_split values agree on every pair", flush=True)

    compare("find_stored", lambda: dev.csr_find(adj, stored), lambda: torch_find(keys, n, stored), args, result)
    compare("find_random", lambda: dev.csr_find(adj, uniform), lambda: torch_find(keys, n, uniform), args, result)
    compare("candidates", lambda: dev.edge_candidates(adj, args.seed, 0, args.pairs), lambda: torch_candidates(keys, n, args.pairs, g), args,
            result)
    del stored, uniform
    torch.cuda.empty_cache()

    # the whole split, as shipped and with the torch candidates in the kernel's place (its key array is kept across rounds)
    kernel_candidates = dev.edge_candidates

    def split_with_torch():
        dev.edge_candidates = lambda a, seed, first, count: torch_candidates(keys, n, count, g)
        try:
            return lp.mask_test_edges(adj, seed=args.seed)
        finally:
            dev.edge_candidates = kernel_candidates

    split_args = argparse.Namespace(reps=args.split_reps, warmup=1)
    compare("split", lambda: lp.mask_test_edges(adj, seed=args.seed), split_with_torch, split_args, result)
    s = lp.mask_test_edges(adj, seed=args.seed)
    result["split_sizes"] = {f: int(getattr(s, f).shape[0]) for f in s._fields[1:]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, sort_keys=True)
            f.write("\n")
    print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()

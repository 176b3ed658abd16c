#!/usr/bin/env python3
"""The sparse x sparse product (device.csr_matmul -> sgl_csr_matmul_rowptr + sgl_csr_matmul_fill) at the shape of a
meta-path: a synthetic paper x author relation of ogbn-mag's size (736 389 x 1 134 649, about 7.1 M distinct entries, power-law
authors: author = floor(n_authors * u^1.5)) multiplied by its transpose, which is paper__to__author__to__paper.

Legs, each after a warm-up, HIP events around the whole call (the host synchronisation and the allocations included):
    ones       device.csr_matmul(values="ones"), what HeteroNodeDataset.sample_by_meta_path runs
    sum        device.csr_matmul(values="sum")
    torch      torch.sparse.mm of the two CSR tensors on the device, where this torch build has it ("did not run" otherwise)
    scipy      a @ b in float32 on the host (a host clock; --host-reps repetitions): the yardstick of the same run
Before anything is timed the device result is compared with scipy's: row pointer and columns equal, values="sum" bit for bit (the
inputs are positive, so scipy prunes nothing).  A mismatch ends the run with a non-zero exit status.  Also printed: how many rows
fall into each row class (by the bound ub = sum of the lengths of B's rows over A's row).

    python tools/bench_csr_matmul.py [--reps 20] [--warmup 3] [--scale 1.0] [--out profiles/csr_matmul.json]

Prints EXP lines and one JSON line.  No number here is an acceptance criterion."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import device as dev  # noqa: E402
from sgl_amd.io import coo_to_csr_device  # noqa: E402


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
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "all": [round(float(v), 3) for v in a]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scales papers, authors and entries (a rehearsal at 0.01 takes seconds)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_matmul.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_csr_matmul.py needs a GPU (nothing here is measured without one)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    n_paper, n_author, n_edges = (max(int(v * args.scale), 8) for v in (736_389, 1_134_649, 7_145_660))
    gen = torch.Generator(device=device)
    gen.manual_seed(args.seed)
    paper = torch.randint(0, n_paper, (n_edges,), device=device, generator=gen)
    author = (torch.rand(n_edges, device=device, generator=gen, dtype=torch.float64) ** 1.5 * n_author).long().clamp_(max=n_author - 1)
    key = torch.unique(paper * n_author + author)
    paper, author = key // n_author, key % n_author
    val = torch.rand(key.numel(), device=device, generator=gen) + 0.5
    a = coo_to_csr_device(paper, author, val, n_paper, device=device, num_col=n_author)
    b = coo_to_csr_device(author, paper, val, n_author, device=device, num_col=n_paper)
    len_b = (b.rowptr[1:] - b.rowptr[:-1]).to(torch.float64)
    ub = torch.zeros(n_paper, dtype=torch.float64, device=device).index_add_(
        0, torch.repeat_interleave(torch.arange(n_paper, device=device), a.rowptr[1:] - a.rowptr[:-1]), len_b[a.col.long()])
    classes = {name: int(((ub >= lo) & (ub <= hi)).sum()) for name, lo, hi in (("empty", 0, 0), ("32", 1, 32), ("128", 33, 128), ("512", 129, 512),
                                                                               ("wide", 513, float("inf")))}
    result = {"papers": n_paper, "authors": n_author, "nnz_a": a.nnz, "longest_author_row": int(len_b.max()), "candidate_products": int(ub.sum()),
              "rows_per_class": classes, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(device)}
    print(f"EXP csr_matmul: {n_paper} x {n_author}, {a.nnz} entries, longest author row {result['longest_author_row']}, "
          f"{result['candidate_products']} candidate products, rows per class {classes}", flush=True)

    sa, sb = a.to_scipy(), b.to_scipy()
    host = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        want = sa @ sb
        host.append((time.perf_counter() - t0) * 1e3)
    want.sort_indices()
    got = dev.csr_matmul(a, b, values="sum")
    same = (np.array_equal(got.rowptr.cpu().numpy(), want.indptr) and np.array_equal(got.col.cpu().numpy(), want.indices)
            and np.array_equal(got.val.cpu().numpy().view(np.uint32), want.data.view(np.uint32)))
    ones = dev.csr_matmul(a, b, values="ones")
    if not (same and torch.equal(ones.col, got.col) and bool((ones.val == 1.0).all())):
        raise SystemExit("bench_csr_matmul.py: the device product and scipy's disagree; nothing was timed")
    result["nnz_c"] = got.nnz
    del got, ones, want

    legs = {"ones": lambda: dev.csr_matmul(a, b, values="ones"), "sum": lambda: dev.csr_matmul(a, b, values="sum")}
    try:
        ta = torch.sparse_csr_tensor(a.rowptr, a.col.long(), a.val, size=a.shape)
        tb = torch.sparse_csr_tensor(b.rowptr, b.col.long(), b.val, size=b.shape)
        torch.sparse.mm(ta, tb)
        torch.cuda.synchronize()
        legs["torch"] = lambda: torch.sparse.mm(ta, tb)
    except Exception as e:                                       # noqa: BLE001  (whatever this build raises: the leg is reported as absent)
        result["torch"] = f"did not run: {type(e).__name__}: {str(e)[:200]}"
        print(f"EXP csr_matmul torch.sparse.mm {result['torch']}", flush=True)
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.reps):                                   # interleaved: all legs see the same drift of the machine
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    result["scipy_ms"] = stats(host)
    for name in legs:
        result[f"{name}_ms"] = stats(ms[name])
    for name in list(legs) + ["scipy"]:
        s = result[f"{name}_ms"]
        print(f"EXP csr_matmul {name}: min {s['min']:.2f}, median {s['median']:.2f}, max {s['max']:.2f} ms; scipy / this = "
              f"{result['scipy_ms']['median'] / s['median']:.1f}", flush=True)
    print(f"EXP csr_matmul: nnz(C) = {result['nnz_c']}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, sort_keys=True)
            f.write("\n")
    print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()

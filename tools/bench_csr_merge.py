#!/usr/bin/env python3
"""The CSR merge (device.csr_merge -> sgl_csr_merge_rowptr + sgl_csr_merge_fill) against the only device route there
was before it: expand the resident CSR to a COO list, concatenate the new entries, and run the ingest again (io.coo_to_csr_device, a
radix sort of every entry already stored).

The graph is the products-shaped synthetic one (synthetic.chung_lu_torch with the S1 parameters: N = 2 449 029, 2 x 61.9 M stored
entries).  Three cases, each timed INTERLEAVED with the re-ingest in one process (warm-up, then --reps repetitions, HIP events around
the whole call -- the merge's host synchronisation and allocations included, and for add_edges / to_undirected the ingest of the
added list / of the transpose, which is part of the public function):
    self_loops   add_self_loops(adj)
    add_1m       add_edges(adj, 1 M random pairs, random weights)
    undirected   to_undirected of the strict upper triangle (taken through device.csr_select); the result must have the structure
                 of the original graph without its diagonal
Before anything is timed the two sides are compared bit for bit (row pointer, columns, and the values wherever a pair occurs at
most twice in the concatenation -- the contract); a mismatch ends the run with a non-zero exit status.

Also timed: the two entry points alone on preallocated outputs and prepared inputs ("entries": count kernel, scan with its scratch
allocation, the read-back of the total, fill kernel), set against the algorithmic bytes at the 6.29 TB/s copy ceiling the project
uses.  The byte model, counted here: the columns of both sides in the count pass (4 B per entry), columns and values of both sides
read (8 B per entry) and the result written (8 B per output entry) in the fill pass, 24 B per row.
Peak temporary bytes of both routes (torch.cuda.max_memory_allocated around each leg; the library's own hipMalloc scratch, O(rows), is
not seen by torch).

The verdict per case: the merge is "faster" (or "slower") only where the medians differ by more than the larger max - min spread of
the two legs; otherwise "no difference shown".

    python tools/bench_csr_merge.py [--reps 20] [--warmup 3] [--workload S1_products] [--out profiles/csr_merge.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_csr_merge.py --only self_loops      # the kernels' own times, one case per run

Prints one JSON line (and writes it to --out).  No number here is an acceptance criterion."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import _lib, device as dev, synthetic, transforms as tr  # noqa: E402
from sgl_amd.io import DeviceAdjacency, coo_to_csr_device  # noqa: E402

COPY_CEILING = 6.29e12      # bytes per second
CASES = ("self_loops", "add_1m", "undirected")


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
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "spread": float(a.max() - a.min()),
            "slowest_repetition": int(a.argmax()), "second_slowest": float(np.sort(a)[-2]) if len(a) > 1 else float(a.max()),
            "all": [round(float(v), 4) for v in a]}


def torch_rows(adj):
    return torch.repeat_interleave(torch.arange(adj.shape[0], dtype=torch.int64, device=adj.device), adj.rowptr[1:] - adj.rowptr[:-1])


def reingest(adj, rows, cols, vals):
    """the route of the parent commit: the stored entries as a COO list, the new ones behind them, the ingest over everything"""
    n = adj.shape[0]
    return coo_to_csr_device(torch.cat((torch_rows(adj), rows)), torch.cat((adj.col.to(torch.int64), cols)), torch.cat((adj.val, vals)), n,
                             device=adj.device)


def entries_only(a, b, mode, out):
    """the two entry points on preallocated outputs"""
    n_rows, n_cols = a.shape
    total = ctypes.c_int64(0)
    dev._call(a.device, "sgl_csr_merge_rowptr", _lib.ptr(a.rowptr), _lib.ptr(a.col), a.nnz, _lib.ptr(b.rowptr), _lib.ptr(b.col), b.nnz, n_rows, n_cols,
              0, _lib.ptr(out[0]), ctypes.byref(total))
    dev._call(a.device, "sgl_csr_merge_fill", _lib.ptr(a.rowptr), _lib.ptr(a.col), _lib.ptr(a.val), a.nnz, _lib.ptr(b.rowptr), _lib.ptr(b.col),
              _lib.ptr(b.val), b.nnz, n_rows, n_cols, mode, 0, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), None, None)
    return total.value


def same_where_the_contract_says(name, ours, theirs, a, list_keys):
    """row pointer and columns exact; values bit-equal except where a pair occurs three times or more in the concatenation"""
    if not (torch.equal(ours.rowptr, theirs.rowptr) and torch.equal(ours.col, theirs.col)):
        raise SystemExit(f"bench_csr_merge.py: the merge and the re-ingest disagree on the structure of {name}; nothing was timed")
    differ = torch.nonzero(ours.val.view(torch.int32) != theirs.val.view(torch.int32)).reshape(-1)
    if differ.numel() == 0:
        return 0
    n = a.shape[0]
    rows = torch.searchsorted(ours.rowptr, differ, right=True) - 1
    cols = ours.col[differ].to(torch.int64)
    in_list = torch.zeros_like(differ)
    if list_keys is not None:
        key = rows * n + cols
        in_list = torch.searchsorted(list_keys, key, right=True) - torch.searchsorted(list_keys, key, right=False)
    stored = (dev.csr_find(a, torch.stack((rows, cols), 1)) >= 0).to(torch.int64)
    if bool(((in_list + stored) <= 2).any()):
        raise SystemExit(f"bench_csr_merge.py: the merge and the re-ingest disagree on a value of {name} whose pair occurs at most twice; "
                         "nothing was timed")
    return int(differ.numel())


def verdict(merge, other):
    gap = abs(merge["median"] - other["median"])
    if gap <= max(merge["spread"], other["spread"]):
        return "no difference shown"
    return "faster" if merge["median"] < other["median"] else "slower"


def measure(name, ours, theirs, a, b, mode, list_keys, args, result):
    x, y = ours(), theirs()
    beyond = same_where_the_contract_says(name, x, y, a, list_keys)
    nnz_out = x.nnz
    del x, y
    n = a.shape[0]
    out = (torch.empty(n + 1, dtype=torch.int64, device=a.device), torch.empty(nnz_out, dtype=torch.int32, device=a.device),
           torch.empty(nnz_out, dtype=torch.float32, device=a.device))
    entries = lambda: entries_only(a, b, mode, out)      # noqa: E731
    assert entries() == nnz_out
    extra_m, extra_r = peak_above_inputs(ours), peak_above_inputs(theirs)
    for _ in range(args.warmup):
        ours()
        theirs()
        entries()
    torch.cuda.synchronize()
    ms_m, ms_r, ms_e = [], [], []
    for _ in range(args.reps):                      # interleaved: all legs see the same drift of the machine
        ms_m.append(timed(ours))
        ms_r.append(timed(theirs))
        ms_e.append(timed(entries))
    sm, sr, se = stats(ms_m), stats(ms_r), stats(ms_e)
    model_bytes = 4 * (a.nnz + b.nnz) + 8 * (a.nnz + b.nnz) + 8 * nnz_out + 24 * n
    share = model_bytes / COPY_CEILING * 1e3 / se["median"]
    v = verdict(sm, sr)
    result[name] = {"merge_ms": sm, "reingest_ms": sr, "entries_ms": se, "ratio_merge_over_reingest": sm["median"] / sr["median"], "verdict": v,
                    "nnz_a": a.nnz, "nnz_b": b.nnz, "nnz_out": nnz_out, "values_beyond_the_contract": beyond,
                    "merge_peak_above_inputs_bytes": extra_m, "reingest_peak_above_inputs_bytes": extra_r, "model_bytes": model_bytes,
                    "entries_share_of_copy_ceiling": share}
    for leg, s in (("merge", sm), ("re-ingest", sr), ("entries", se)):
        print(f"EXP csr_merge {name} {leg}: min {s['min']:.3f}, median {s['median']:.3f}, second slowest {s['second_slowest']:.3f}, slowest {s['max']:.3f} ms "
              f"(repetition {s['slowest_repetition']} of {args.reps})", flush=True)
    print(f"EXP csr_merge {name}: {a.nnz} + {b.nnz} -> {nnz_out} entries ({beyond} values of pairs listed three times or more differ); merge "
          f"{sm['median']:.3f} ms (spread {sm['spread']:.3f}), re-ingest {sr['median']:.3f} ms (spread {sr['spread']:.3f}), ratio "
          f"{sm['median'] / sr['median']:.3f}: {v}; entries alone {se['median']:.3f} ms (spread {se['spread']:.3f}) = {share:.3f} of the copy ceiling "
          f"for {model_bytes / 2**20:.0f} MiB; peak above inputs {extra_m / 2**20:.0f} against {extra_r / 2**20:.0f} MiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="S1_products")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--only", default="", help="one case (self_loops, add_1m or undirected) and nothing else: for a kernel trace in a run of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_merge.json"))
    args = ap.parse_args()
    if args.only not in ("",) + CASES:
        raise SystemExit(f"bench_csr_merge.py: --only takes one of {CASES}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_csr_merge.py needs a GPU (nothing here is measured without one)")
    if args.reps < 20:
        print("EXP csr_merge: fewer than 20 repetitions: not a measurement to quote", flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    w = synthetic.WORKLOADS[args.workload]
    n = w["n"]
    adj = DeviceAdjacency(*synthetic.chung_lu_torch(n, w["m"], w["d_max"], seed=args.seed, device=device), (n, n))
    result = {"workload": args.workload, "n": n, "nnz": adj.nnz, "reps": args.reps, "warmup": args.warmup, "copy_ceiling_bytes_per_s": COPY_CEILING,
              "device": torch.cuda.get_device_name(device)}
    print(f"EXP csr_merge {args.workload}: n = {n}, nnz = {adj.nnz}", flush=True)
    ids = torch.arange(n, dtype=torch.int64, device=device)

    if args.only in ("", "self_loops"):
        ones = torch.ones(n, dtype=torch.float32, device=device)
        eye = DeviceAdjacency(torch.arange(n + 1, dtype=torch.int64, device=device), ids.to(torch.int32), ones, (n, n))
        measure("self_loops", lambda: tr.add_self_loops(adj), lambda: reingest(adj, ids, ids, ones), adj, eye, _lib.SGL_MERGE_SUM, None, args, result)
        del eye

    if args.only in ("", "add_1m"):
        gen = torch.Generator(device=device)
        gen.manual_seed(args.seed + 1)
        pairs = torch.randint(0, n, (2, args.pairs), device=device, generator=gen)
        weights = torch.rand(args.pairs, device=device, generator=gen) + 0.5
        added = coo_to_csr_device(pairs[0], pairs[1], weights, n, device=device)
        list_keys = torch.sort(pairs[0] * n + pairs[1]).values
        measure("add_1m", lambda: tr.add_edges(adj, pairs, weights), lambda: reingest(adj, pairs[0], pairs[1], weights), adj, added, _lib.SGL_MERGE_SUM,
                list_keys, args, result)
        result["add_1m"]["pairs"] = args.pairs
        del added, list_keys

    if args.only in ("", "undirected"):
        rows = torch_rows(adj)
        upper = dev.csr_select(adj, entry_keep=(adj.col.to(torch.int64) > rows))
        del rows
        urows = torch_rows(upper)
        ucols = upper.col.to(torch.int64)
        mirror = coo_to_csr_device(ucols, urows, upper.val, n, device=device)
        whole = tr.to_undirected(upper)
        original = dev.csr_select(adj, drop_self=True)
        if not (torch.equal(whole.rowptr, original.rowptr) and torch.equal(whole.col, original.col)):
            raise SystemExit("bench_csr_merge.py: to_undirected of the upper triangle does not have the structure of the original graph")
        result["stored_diagonal_entries"] = adj.nnz - original.nnz
        del whole, original
        measure("undirected", lambda: tr.to_undirected(upper), lambda: reingest(upper, ucols, urows, upper.val), upper, mirror, _lib.SGL_MERGE_SUM, None,
                args, result)

    if args.out and not args.only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, sort_keys=True)
            f.write("\n")
    print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()

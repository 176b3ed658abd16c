#!/usr/bin/env python3
"""The CSR select (device.csr_select -> sgl_csr_select_rowptr + sgl_csr_select_fill) against the torch composition a
user had before it, on the device: row ids by repeat_interleave, the predicate as tensor expressions, boolean indexing of the three
arrays, bincount and cumsum for the new row pointer.

The graph is the products-shaped synthetic one (synthetic.chung_lu_torch with the S1 parameters: N = 2 449 029, 2 x 61.9 M stored
entries).  Three selections, each timed INTERLEAVED with its torch composition in one process (warm-up, then --reps repetitions, HIP
events around the whole call -- the select's host synchronisation and allocations included):
    nodes_8     get_subgraph with a node mask that keeps 8 % of the nodes (the training share of ogbn-products)
    nodes_50    get_subgraph with a node mask that keeps 50 %
    edges_sym   random_drop_edges(p = 0.5, force_undirected=True); the torch side computes the same hash with int64 tensor arithmetic
Before anything is timed the two sides are compared bit for bit (row pointer, columns, values); a mismatch ends the run with a
non-zero exit status.

Also timed: the two entry points alone on preallocated outputs ("entries": count kernel, memset, scan with its scratch allocation,
the read-back of the total, fill kernel), set against the algorithmic bytes at the 6.29 TB/s copy ceiling the project uses.  The byte
model, counted here: 4 B per entry in the count pass, 8 B per entry read plus 8 B per kept entry written in the fill pass, 16 B per
row.  It charges every entry; rows that the row map drops are in fact never read, so a node selection can come out above 1.
And one scipy a[m][:, m] on the HOST with the upload of the result (DeviceAdjacency.from_scipy), at --host-workload (S1_small:
200 000 nodes, about 10 M entries), mask 50 %.

    python tools/bench_csr_select.py [--reps 20] [--warmup 3] [--workload S1_products] [--out profiles/csr_select.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_csr_select.py --only nodes_50     # the kernels' own times, one selection per run

Prints one JSON line (and writes it to --out).  No number here is an acceptance criterion."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import _lib, device as dev, synthetic, transforms as tr  # noqa: E402
from sgl_amd.io import DeviceAdjacency  # noqa: E402
from sgl_amd.tricks.link_prediction import _hash4, _u64  # noqa: E402

COPY_CEILING = 6.29e12      # bytes per second


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


def torch_rows(adj):
    return torch.repeat_interleave(torch.arange(adj.shape[0], dtype=torch.int64, device=adj.device), adj.rowptr[1:] - adj.rowptr[:-1])


def torch_compact(adj, rows, cols, keep, n_out):
    r, c, v = rows[keep], cols[keep], adj.val[keep]
    rowptr = torch.zeros(n_out + 1, dtype=torch.int64, device=adj.device)
    torch.cumsum(torch.bincount(r, minlength=n_out), 0, out=rowptr[1:])
    return rowptr, c.to(torch.int32), v


def torch_subgraph(adj, mask):
    rows, cols = torch_rows(adj), adj.col.to(torch.int64)
    keep = mask[rows] & mask[cols]
    new = torch.cumsum(mask, 0) - 1
    return torch_compact(adj, new[rows], new[cols], keep, int(mask.sum()))


def torch_edge_drop(adj, p, seed):
    rows, cols = torch_rows(adj), adj.col.to(torch.int64)
    h = _hash4(seed, tr.EDGE_DROP_STREAM, torch.minimum(rows, cols), torch.maximum(rows, cols))
    keep = (h ^ _u64(1 << 63)) >= (_u64(tr.drop_threshold(p)) ^ _u64(1 << 63))
    return torch_compact(adj, rows, cols, keep, adj.shape[0])


def entries_only(adj, select, n_rows_out, out):
    """the two entry points on preallocated outputs; select: the eleven selection arguments"""
    n_rows, n_cols = adj.shape
    total = ctypes.c_int64(0)
    dev._call(adj.device, "sgl_csr_select_rowptr", _lib.ptr(adj.rowptr), _lib.ptr(adj.col), n_rows, n_cols, adj.nnz, *select, _lib.ptr(out[0]),
              ctypes.byref(total))
    dev._call(adj.device, "sgl_csr_select_fill", _lib.ptr(adj.rowptr), _lib.ptr(adj.col), _lib.ptr(adj.val), n_rows, n_cols, adj.nnz, *select,
              _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), None)
    return total.value


def compare(name, ours, theirs, entries, kept, adj, args, result):
    a, b = ours(), theirs()
    if not (torch.equal(a.rowptr, b[0]) and torch.equal(a.col, b[1]) and torch.equal(a.val.view(torch.int32), b[2].view(torch.int32))):
        raise SystemExit(f"bench_csr_select.py: the select disagrees with the torch composition on {name}; nothing was timed")
    assert a.nnz == kept
    del a, b
    extra_k, extra_t = peak_above_inputs(ours), peak_above_inputs(theirs)
    for _ in range(args.warmup):
        ours()
        theirs()
        entries()
    torch.cuda.synchronize()
    ms_k, ms_t, ms_e = [], [], []
    for _ in range(args.reps):                      # interleaved: all sides see the same drift of the machine
        ms_k.append(timed(ours))
        ms_t.append(timed(theirs))
        ms_e.append(timed(entries))
    sk, st, se = stats(ms_k), stats(ms_t), stats(ms_e)
    model_bytes = 4 * adj.nnz + 8 * adj.nnz + 8 * kept + 16 * adj.shape[0]
    share = model_bytes / COPY_CEILING * 1e3 / se["median"]
    result[name] = {"select_ms": sk, "torch_ms": st, "entries_ms": se, "ratio_select_over_torch": sk["median"] / st["median"], "kept_entries": kept,
                    "select_peak_above_inputs_bytes": extra_k, "torch_peak_above_inputs_bytes": extra_t, "model_bytes": model_bytes,
                    "entries_share_of_copy_ceiling": share}
    print(f"EXP csr_select {name}: kept {kept} of {adj.nnz}; select {sk['median']:.3f} ms ({sk['min']:.3f}-{sk['max']:.3f}), torch "
          f"{st['median']:.3f} ms ({st['min']:.3f}-{st['max']:.3f}), ratio {sk['median'] / st['median']:.3f}; entries alone {se['median']:.3f} ms "
          f"({se['min']:.3f}-{se['max']:.3f}) = {share:.3f} of the copy ceiling for {model_bytes / 2**20:.0f} MiB; peak above inputs "
          f"{extra_k / 2**20:.0f} against {extra_t / 2**20:.0f} MiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="S1_products")
    ap.add_argument("--host-workload", default="S1_small")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="", help="one selection (nodes_8, nodes_50 or edges_sym) and nothing else: for a kernel trace in a run of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_select.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_csr_select.py needs a GPU (nothing here is measured without one)")
    if args.reps < 20:
        print("EXP csr_select: fewer than 20 repetitions: not a measurement to quote", flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    w = synthetic.WORKLOADS[args.workload]
    n = w["n"]
    adj = DeviceAdjacency(*synthetic.chung_lu_torch(n, w["m"], w["d_max"], seed=args.seed, device=device), (n, n))
    result = {"workload": args.workload, "n": n, "nnz": adj.nnz, "reps": args.reps, "warmup": args.warmup, "copy_ceiling_bytes_per_s": COPY_CEILING,
              "device": torch.cuda.get_device_name(device)}
    print(f"EXP csr_select {args.workload}: n = {n}, nnz = {adj.nnz}", flush=True)
    out = (torch.empty(n + 1, dtype=torch.int64, device=device), torch.empty(adj.nnz, dtype=torch.int32, device=device),
           torch.empty(adj.nnz, dtype=torch.float32, device=device))

    for name, share in (("nodes_8", 0.08), ("nodes_50", 0.5)):
        if args.only not in ("", name):
            continue
        mask = tr.node_keep_mask(n, 1.0 - share, seed=args.seed + 1, device=device)
        k = int(mask.sum())
        id_map = torch.where(mask, torch.cumsum(mask, 0, dtype=torch.int32) - 1, -1).to(torch.int32).contiguous()
        select = (_lib.ptr(id_map), _lib.ptr(id_map), k, k, None, 0, 0, 0, 0, 0, 0)
        kept = entries_only(adj, select, k, out)
        compare(name, lambda: tr.get_subgraph(adj, mask).adj, lambda: torch_subgraph(adj, mask), lambda: entries_only(adj, select, k, out), kept, adj,
                args, result)
        result[name]["kept_nodes"] = k
    if args.only not in ("", "edges_sym"):
        print(json.dumps(result, sort_keys=True), flush=True)
        return
    t = tr.drop_threshold(0.5)
    select = (None, None, n, n, None, 0, 0, t, args.seed, 1, 0)
    kept = entries_only(adj, select, n, out)
    compare("edges_sym", lambda: tr.random_drop_edges(adj, p=0.5, force_undirected=True, seed=args.seed), lambda: torch_edge_drop(adj, 0.5, args.seed),
            lambda: entries_only(adj, select, n, out), kept, adj, args, result)
    if args.only:
        print(json.dumps(result, sort_keys=True), flush=True)
        return
    for lanes in dev.CSR_SELECT_LANES:              # the instance the mean row length does not pick, for the record
        sel = select[:-1] + (lanes,)
        entries_only(adj, sel, n, out)
        result.setdefault("edges_sym_entries_ms_by_lanes", {})[str(lanes)] = stats([timed(lambda: entries_only(adj, sel, n, out)) for _ in range(args.reps)])
    print(f"EXP csr_select edges_sym entries alone by lanes: "
          + ", ".join(f"{k}: {v['median']:.3f} ms" for k, v in result["edges_sym_entries_ms_by_lanes"].items()), flush=True)
    del out, adj
    torch.cuda.empty_cache()

    # the route this replaces, on the host: scipy's a[m][:, m] and the upload of the result
    hw = synthetic.WORKLOADS[args.host_workload]
    indptr, indices, data = synthetic.chung_lu_numpy(hw["n"], hw["m"], hw["d_max"], seed=args.seed)
    import scipy.sparse as sp
    a = sp.csr_matrix((data, indices, indptr), shape=(hw["n"], hw["n"]))
    m = np.random.default_rng(args.seed).random(hw["n"]) < 0.5
    host_adj = DeviceAdjacency.from_scipy(a, device=device)
    dmask = torch.from_numpy(m).to(device)
    tr.get_subgraph(host_adj, dmask)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sub = a[m][:, m]
    t1 = time.perf_counter()
    up = DeviceAdjacency.from_scipy(sub, device=device)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    ours = tr.get_subgraph(host_adj, dmask).adj
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    assert torch.equal(ours.rowptr, up.rowptr) and torch.equal(ours.col, up.col)
    result["host_scipy"] = {"workload": args.host_workload, "n": hw["n"], "nnz": int(a.nnz), "kept_entries": int(sub.nnz), "scipy_ms": (t1 - t0) * 1e3,
                            "upload_ms": (t2 - t1) * 1e3, "device_select_wall_ms": (t3 - t2) * 1e3}
    print(f"EXP csr_select host route at {args.host_workload} (n = {hw['n']}, nnz = {a.nnz}, mask 50 %): scipy a[m][:, m] {(t1 - t0) * 1e3:.1f} ms + upload "
          f"{(t2 - t1) * 1e3:.1f} ms (one run each); get_subgraph on the device {(t3 - t2) * 1e3:.2f} ms wall", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, sort_keys=True)
            f.write("\n")
    print(json.dumps(result, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()

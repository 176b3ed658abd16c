#!/usr/bin/env python3
"""The 'jk' aggregator's forward + backward on stored hop rows (K24) against the gathered route of the parent commit (gather_hops,
then the float32 kernels): S1 row count, B = 50 000, H = 6, d in {100, 147}, float32 and bfloat16 tables.  The two legs run
interleaved in one process, after a warm-up; sampled rows of the two results are compared first.  Writes medians and ranges to
profiles/hop_rows.json.

    python tools/bench_hop_rows.py [--rows 2449029] [--batch 50000] [--reps 30] [--warmup 5] [--out profiles/hop_rows.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgl_amd import device as dev  # noqa: E402
from sgl_amd.operators.message_op import LearnableWeightedMessageOp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_449_029)
    ap.add_argument("--batch", type=int, default=50_000)
    ap.add_argument("--hops", type=int, default=6)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "hop_rows.json"))
    a = ap.parse_args()
    cuda = torch.device("cuda", 0)
    results = []
    for d in (100, 147):
        for dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(d)
            tabs = []
            for _ in range(a.hops):
                t = dev.alloc_rows(a.rows, d, cuda, dtype=dtype)
                t.copy_(torch.randn((a.rows, d), device=cuda))
                tabs.append(t)
            idx = torch.randint(0, a.rows, (a.batch,), device=cuda)
            g = torch.randn((a.batch, d), device=cuda)
            op = LearnableWeightedMessageOp(0, a.hops, "jk", a.hops - 1, d).to(cuda)
            legs = {"in_place": lambda: op.aggregate_rows(tabs, idx), "gathered": lambda: op.aggregate(dev.gather_hops(tabs, idx))}
            outs = {k: f().detach() for k, f in legs.items()}
            sample = torch.arange(0, a.batch, max(1, a.batch // 512), device=cuda)
            if not torch.equal(outs["in_place"][sample], outs["gathered"][sample]):
                raise SystemExit(f"d={d} {dtype}: the sampled rows of the two routes differ")
            times = {k: [] for k in legs}
            for rep in range(a.warmup + a.reps):
                for k, f in legs.items():                              # interleaved: both legs see the same clocks and caches
                    op.zero_grad()
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    f().backward(g)
                    stop.record()
                    stop.synchronize()
                    if rep >= a.warmup:
                        times[k].append(start.elapsed_time(stop))
            row = {"d": d, "dtype": str(dtype).replace("torch.", ""), "rows": a.rows, "batch": a.batch, "hops": a.hops, "reps": a.reps}
            for k, ts in times.items():
                row[k + "_ms"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
            row["in_place_over_gathered"] = row["in_place_ms"]["median"] / row["gathered_ms"]["median"]
            print(json.dumps(row), flush=True)
            results.append(row)
            del tabs
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump({"workload": "jk aggregator forward + backward, wall time per step between two events", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()

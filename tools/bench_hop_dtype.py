#!/usr/bin/env python3
"""fp32 against bfloat16 hop storage (GraphOp(hop_dtype="bfloat16")) on the BASELINE config 2 workload: the
ogbn-products-shaped Chung-Lu graph of the bench (same generator, same seed), LaplacianGraphOp r = 0.5, k = 3 hops per step.

One process, the variants INTERLEAVED step by step (every step = the k-hop chain of one variant, timed with device events), after
a warm-up of every variant: fp32 hops (the kernel of the default path, unchanged), bf16 hops at d = 100 with both candidate row
pitches (104 and 128 elements), and fp32 / bf16 at d = 128 and d = 147.  Prints the medians and the spread, writes
profiles/bf16_hop_dtype.json (--out) and says which d = 100 pitch is faster.

Before anything is timed, one hop of every variant is checked on sampled rows (the longest included), bit for bit, against the CPU
model of the kernels' default summation order (oracle.oracle_spmm_slots with the R of the kernel the dispatch rule picks,
tests/spmm_order_common.py).  A mismatch ends the run with a non-zero exit status: no ratio comes from an unchecked kernel.

    python tools/bench_hop_dtype.py [--steps 20] [--warmup 3] [--workload S1_products] [--out profiles/bf16_hop_dtype.json]

Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_hop_dtype.py --steps 3 --out ''` for kernel times, and under
`rocprofv3 --pmc TCC_REQ_sum TCC_READ_sum -- ...` (no tracing in that run) for the L2 request counts of the two kernels."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
from sgl_amd import _lib, device as dev, synthetic  # noqa: E402
from spmm_order_common import default_long_row_nnz, dispatch  # noqa: E402

K = 3


def padded(n, d, ld, dtype, device):
    """[n, ld] buffer whose first d columns are data and whose pad columns are zero"""
    buf = torch.zeros((n, ld), dtype=dtype, device=device)
    return buf


class Variant:
    def __init__(self, name, csr, x, d, ld, dtype, unroll=0):
        n = x.shape[0]
        self.name, self.csr, self.d, self.ld, self.dtype, self.unroll = name, csr, d, ld, dtype, unroll
        self.x = padded(n, d, ld, dtype, x.device)
        self.x[:, :d].copy_(x[:, :d])
        self.outs = [padded(n, d, ld, dtype, x.device) for _ in range(K)]
        self.ms = []

    def step(self):
        if self.unroll:                      # experiment: another number of gathers in flight (tuning key "spmm_unroll")
            _lib.set_tuning("spmm_unroll", self.unroll)
        self.csr.spmm_chain(self.x, K, outs=self.outs)
        if self.unroll:
            _lib.set_tuning("spmm_unroll", 0)

    def check(self, host_csr, rows):
        """one hop against the model on `rows`: number of elements whose bits differ (0 = checked and equal)"""
        import oracle  # the checker: the CPU model of the kernels' summation order, never part of what is timed
        rp, cc, vv = host_csr
        n, bf16 = len(rp) - 1, self.dtype == torch.bfloat16
        y = self.outs[0]
        tuning = {"spmm_unroll": self.unroll} if self.unroll else {}
        slices = dispatch("bf16" if bf16 else "f32", self.x.shape[1], self.x.stride(0), y.stride(0), self.x.data_ptr(), y.data_ptr(),
                          False, len(cc) / n, tuning)
        for k, val in tuning.items():
            _lib.set_tuning(k, val)
        try:
            self.csr.spmm(self.x, out=y)
        finally:
            for k in tuning:
                _lib.set_tuning(k, 0)
        xh = self.x.cpu().float().numpy()
        lr = default_long_row_nnz(len(cc))
        want = np.empty((len(rows), xh.shape[1]), np.float32)
        for c0, dc, var in slices:
            want[:, c0:c0 + dc] = oracle.oracle_spmm_slots(rp, cc, vv, xh[:, c0:c0 + dc], 64 // var[1], lr, rows=rows)
        got = y[torch.from_numpy(rows).to(y.device)].cpu()
        if bf16:
            w = torch.from_numpy(want).to(torch.bfloat16).view(torch.int16).numpy()
            return int((got.view(torch.int16).numpy() != w).sum()), slices
        return int((got.numpy().view(np.uint32) != want.view(np.uint32)).sum()), slices

    def timed(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.step()
        e1.record()
        torch.cuda.synchronize()
        self.ms.append(e0.elapsed_time(e1) / K)

    def summary(self):
        a = np.asarray(self.ms)
        return {"ms_per_hop_median": float(np.median(a)), "ms_per_hop_min": float(a.min()), "ms_per_hop_max": float(a.max()),
                "ms_per_hop_iqr": float(np.percentile(a, 75) - np.percentile(a, 25)), "steps": int(a.size), "d": self.d,
                "row_pitch_elements": self.ld, "row_bytes": self.ld * dev._esize(self.dtype),
                "expected_lines_per_row": dev.expected_lines(self.ld, self.d, dev._esize(self.dtype)), "dtype": str(self.dtype)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="S1_products")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dims", default="100,128,147")
    ap.add_argument("--bf16-unroll", default="", help="experiment: extra bf16 variants with these spmm_unroll levels (1 = low, 3 = mid, 2 = high)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_hop_dtype.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hop_dtype.py needs a GPU (nothing here is measured without one)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    wl = synthetic.WORKLOADS[args.workload]
    n = wl["n"]
    a_ptr, a_col, a_val = synthetic.chung_lu_torch(n, wl["m"], wl["d_max"], seed=args.seed, device=device)
    rowptr, col, val = dev.normalize_adj(a_ptr, a_col, a_val, n, 0.5, None)
    del a_ptr, a_col, a_val
    csr = dev.DeviceCSR(rowptr, col, val, (n, n))
    host_csr = (rowptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy())
    deg = np.diff(host_csr[0])
    check_rows = np.unique(np.concatenate([np.random.default_rng(args.seed).choice(n, min(n, 2047), replace=False),
                                           [int(deg.argmax())]])).astype(np.int64)
    result = {"workload": args.workload, "n_nodes": n, "nnz_a_hat": int(col.numel()), "prop_steps": K, "steps": args.steps,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(device), "variants": {}, "ratios_bf16_over_fp32": {}}
    for d in [int(v) for v in args.dims.split(",")]:
        x = synthetic.features_torch(n, d, seed=args.seed, device=device)
        variants = [Variant(f"d{d}_fp32", csr, x, d, dev.row_pitch(d), torch.float32)]
        pitches = sorted({dev.round_up(d, 8), dev.round_up(d, 64), dev.row_pitch(d, elem_size=2)}) if d == 100 else [dev.row_pitch(d, elem_size=2)]
        for ld in pitches:
            variants.append(Variant(f"d{d}_bf16_pitch{ld}", csr, x, d, ld, torch.bfloat16))
            for un in [int(v) for v in args.bf16_unroll.split(",") if v]:
                variants.append(Variant(f"d{d}_bf16_pitch{ld}_unroll{un}", csr, x, d, ld, torch.bfloat16, unroll=un))
        del x
        for v in variants:                     # values first: a ratio from a kernel that computes something else is worth nothing
            n_bad, slices = v.check(host_csr, check_rows)
            print(f"EXP hop_dtype {v.name}: {len(check_rows)} sampled rows of one hop against the model: "
                  f"{'bit-equal' if n_bad == 0 else f'{n_bad} ELEMENTS DIFFER'} (kernel {[s_[2] for s_ in slices]})", flush=True)
            if n_bad:
                raise SystemExit(f"bench_hop_dtype.py: {v.name} does not compute the documented sums; nothing was timed")
        for _ in range(args.warmup):
            for v in variants:
                v.step()
        torch.cuda.synchronize()
        for _ in range(args.steps):
            for v in variants:                 # interleaved: every variant sees the same drift of the machine
                v.timed()
        base = None
        for v in variants:
            s = v.summary()
            result["variants"][v.name] = s
            if v.dtype == torch.float32:
                base = s["ms_per_hop_median"]
            else:
                result["ratios_bf16_over_fp32"][v.name] = s["ms_per_hop_median"] / base
            print(f"EXP hop_dtype {v.name}: ms_per_hop median={s['ms_per_hop_median']:.3f} min={s['ms_per_hop_min']:.3f} "
                  f"max={s['ms_per_hop_max']:.3f} iqr={s['ms_per_hop_iqr']:.3f} pitch={v.ld} lines/row={s['expected_lines_per_row']:.2f}"
                  + ("" if v.dtype == torch.float32 else f" ratio_to_fp32={s['ms_per_hop_median'] / base:.3f}"), flush=True)
        del variants
        torch.cuda.empty_cache()
    cands = {k: v["ms_per_hop_median"] for k, v in result["variants"].items() if k.startswith("d100_bf16_pitch")}
    if cands:
        best = min(cands, key=cands.get)
        result["d100_faster_pitch"] = result["variants"][best]["row_pitch_elements"]
        result["d100_row_pitch_default"] = dev.row_pitch(100, elem_size=2)
        print(f"EXP hop_dtype d=100: faster bf16 pitch = {result['d100_faster_pitch']} elements "
              f"(row_pitch(100, elem_size=2) = {result['d100_row_pitch_default']})", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"EXP hop_dtype wrote {args.out}", flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The fused linear head (DESIGN K21) against the torch head it replaces, on one MI355X.

    python tools/bench_head.py [--reps 20 --warmup 3 --out profiles/linear_head.json]

Shapes: N = 2 449 029 (all nodes) and 196 615 (the products train split), (d, C) = (100, 47), (128, 172), (500, 3).  Every leg's two
candidates are interleaved in one process, 3 warm-ups + 20 repetitions, HIP events, median (min - max):
  (a) forward + loss + dZ: device.linear_class_loss against F.linear + device.class_loss_grad (K14);
  (b) a whole step with dW and db: linear_cross_entropy + backward against cross_entropy(F.linear(...)) + backward (torch autograd);
  (c) evaluation: the arg-max-only launch against F.linear + predict;
  (d) one read of X at the copy ceiling, the yardstick.
Before timing, the fused outputs of 64 sampled rows are checked against float64 inside the header's bounds.  The comparison point is the
torch path of the same process; nothing is compared against itself.

    python tools/bench_head.py --in-place [--out profiles/linear_head_rows.json]

The head on stored rows (DESIGN K22) against ITS parent path, gather_rows + K21, in the same process and by the same method: a table
of N = 2 449 029 rows, float32 and bfloat16, m = 196 615 random rows through a device index and m = N through idx=None (bfloat16
only: a float32 table without an index is K21's own matrix, and the parent path reads it as a view).  Legs: (a) forward + loss + dZ,
(b) a whole step -- the gather is part of the parent's step --, (c) evaluation, (d) one read of the gathered bytes m d e, (e) the
weight gradient on its own: in place against K21's on a copy gathered beforehand (the parent pays for that copy in its forward).
--rows: the largest entry is the table, every entry a batch size m.

    python tools/bench_head.py --one-pass [--out profiles/linear_head_step.json]

The one-pass step (DESIGN K23) against ITS parent paths, same process, same method, (d, C) = (100, 47) and (200, 3), a table of
N = 2 449 029 rows in float32 and bfloat16, m = 196 615 random rows and m = N.  Leg (f), a whole step = linear_cross_entropy + backward
(autograd and the float64 loss sum included, no optimizer): (f1) one_pass=True on the batch matrix against the K21 step on it -- the
gather is part of both steps, and a float32 table with m = N is the matrix itself --; (f2) one_pass=True with rows= against the K22
in-place step.  Before timing, loss and pred of 64 sampled rows and dW, db are checked against float64."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sgl_amd import _lib, device as dev  # noqa: E402
from sgl_amd.tricks import classification as cl  # noqa: E402

COPY_CEILING_BYTES_PER_S = 6.29e12
SHAPES = ((100, 47), (128, 172), (500, 3))
ROWS = (2449029, 196615)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "linear_head.json")


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
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def compare(fused, torch_path, args, tag, names=("fused", "torch")):
    for _ in range(args.warmup):
        fused()
        torch_path()
    torch.cuda.synchronize()
    ms_f, ms_t = [], []
    for _ in range(args.reps):                     # interleaved: both candidates see the same drift of the machine
        ms_f.append(timed(fused))
        ms_t.append(timed(torch_path))
    sf, st = stats(ms_f), stats(ms_t)
    ratio = sf["median"] / st["median"]
    r = {f"{names[0]}_ms": sf, f"{names[1]}_ms": st, f"ratio_{names[0]}_over_{names[1]}": ratio,
         "expectation_lower_time": "confirmed" if sf["max"] < st["min"] else ("refuted" if sf["min"] > st["max"] else "undecided")}
    print(f"EXP head {tag}: {names[0]} {sf['median']:.3f} ms ({sf['min']:.3f}-{sf['max']:.3f}), {names[1]} {st['median']:.3f} ms "
          f"({st['min']:.3f}-{st['max']:.3f}), ratio {ratio:.3f} {r['expectation_lower_time']}", flush=True)
    return r


def check_sample(x, w, b, y, dz, loss, pred):
    """64 sampled rows against float64 inside the header's bounds; raises on a miss"""
    rows = torch.linspace(0, x.shape[0] - 1, 64, device=x.device).long()
    d, c = x.shape[1], w.shape[0]
    x64, w64 = x[rows].double().cpu().numpy(), w.double().cpu().numpy()
    z = x64 @ w64.T + b.double().cpu().numpy()
    e = ((d + 3) * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T + np.abs(b.cpu().numpy()))).max(1)
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    p, yy = np.exp(z - lse[:, None]), y[rows].cpu().numpy()
    want = lse - z[np.arange(64), yy]
    onehot = np.zeros_like(z)
    onehot[np.arange(64), yy] = 1
    assert (np.abs(loss[rows].cpu().numpy() - want) <= 2 * e + (c + 16) * 2.0 ** -23 + 2.0 ** -23 * (np.abs(lse) + np.abs(want))).all()
    tol = p * (np.expm1(2 * e)[:, None] + (c + 8 + np.abs(z - m[:, None])) * 2.0 ** -23) + 2.0 ** -23
    assert (np.abs(dz[rows].cpu().numpy() - (p - onehot)) <= tol).all()
    assert (z[np.arange(64), pred[rows].cpu().numpy()] >= m - 2 * e).all()


def one_shape(n, d, c, args):
    dev_ = torch.device("cuda", 0)
    gen = torch.Generator(device=dev_).manual_seed(args.seed)
    x = dev.alloc_rows(n, d, dev_)
    x.copy_(torch.randn((n, d), generator=gen, device=dev_))
    lin = torch.nn.Linear(d, c).to(dev_)
    w, b = lin.weight, lin.bias
    y = torch.randint(0, c, (n,), generator=gen, device=dev_)
    dz_buf, z_buf = dev.alloc_rows(n, c, dev_), dev.alloc_rows(n, c, dev_)
    wd, bd = w.detach(), b.detach()
    dz, loss, pred, _ = dev.linear_class_loss(x, wd, bd, y, 1.0, dz=dz_buf, row_loss=True, pred=True)
    check_sample(x, wd, bd, y, dz, loss, pred)
    out = {"n": n, "d": d, "c": c}

    def torch_fwd():
        z = torch.addmm(bd, x, wd.t(), out=z_buf) if z_buf.is_contiguous() else F.linear(x, wd, bd)
        return dev.class_loss_grad(z, y, 1.0, dz=dz_buf, row_loss=True, pred=True)

    out["a_forward_loss_dz"] = compare(lambda: dev.linear_class_loss(x, wd, bd, y, 1.0, dz=dz_buf, row_loss=True, pred=True), torch_fwd, args,
                                       f"(a) n={n} d={d} C={c}")

    def step(fused):
        lin.zero_grad(set_to_none=True)
        loss_ = cl.linear_cross_entropy(x, w, b, y, check=False) if fused else cl.cross_entropy(F.linear(x, w, b), y, check=False)
        loss_.backward()
        return loss_

    out["b_whole_step"] = compare(lambda: step(True), lambda: step(False), args, f"(b) n={n} d={d} C={c}")
    out["c_evaluation"] = compare(lambda: dev.linear_class_loss(x, wd, bd, None, 1.0, pred=True), lambda: cl.predict(F.linear(x, wd, bd)), args,
                                  f"(c) n={n} d={d} C={c}")
    out["d_one_read_of_x_ms"] = n * d * 4 / COPY_CEILING_BYTES_PER_S * 1e3
    return out


def one_table(n_rows, m, d, c, dtype, args):
    """the in-place head on rows of a stored table against gather_rows + K21"""
    dev_ = torch.device("cuda", 0)
    gen = torch.Generator(device=dev_).manual_seed(args.seed)
    table = dev.alloc_rows(n_rows, d, dev_, dtype=dtype)
    table.copy_(torch.randn((n_rows, d), generator=gen, device=dev_))
    idx = None if m == n_rows else torch.randint(0, n_rows, (m,), generator=gen, device=dev_)
    at = torch.arange(n_rows, device=dev_) if idx is None else idx       # the parent's index lives on the device too: no upload is timed
    lin = torch.nn.Linear(d, c).to(dev_)
    w, b = lin.weight, lin.bias
    wd, bd = w.detach(), b.detach()
    y = torch.randint(0, c, (m,), generator=gen, device=dev_)
    dz_buf = dev.alloc_rows(m, c, dev_)
    dz, loss, pred, _ = dev.linear_class_loss_rows(table, idx, wd, bd, y, 1.0, dz=dz_buf, row_loss=True, pred=True)
    check_sample(dev.gather_rows(table, at), wd, bd, y, dz, loss, pred)
    names = ("in_place", "gathered")
    tag = f"n_rows={n_rows} m={m} d={d} C={c} {str(dtype).replace('torch.', '')}"
    out = {"n_rows": n_rows, "m": m, "index": "none" if idx is None else "random", "d": d, "c": c, "dtype": str(dtype).replace("torch.", "")}
    out["a_forward_loss_dz"] = compare(lambda: dev.linear_class_loss_rows(table, idx, wd, bd, y, 1.0, dz=dz_buf, row_loss=True, pred=True),
                                       lambda: dev.linear_class_loss(dev.gather_rows(table, at), wd, bd, y, 1.0, dz=dz_buf, row_loss=True, pred=True),
                                       args, f"(a) {tag}", names)

    def step(in_place):
        lin.zero_grad(set_to_none=True)
        if in_place:
            loss_ = cl.linear_cross_entropy(table, w, b, y, check=False, rows=range(n_rows) if idx is None else idx)
        else:
            loss_ = cl.linear_cross_entropy(dev.gather_rows(table, at), w, b, y, check=False)
        loss_.backward()
        return loss_

    out["b_whole_step"] = compare(lambda: step(True), lambda: step(False), args, f"(b) {tag}", names)
    out["c_evaluation"] = compare(lambda: dev.linear_class_loss_rows(table, idx, wd, bd, None, 1.0, pred=True),
                                  lambda: dev.linear_class_loss(dev.gather_rows(table, at), wd, bd, None, 1.0, pred=True), args, f"(c) {tag}", names)
    out["d_one_read_of_the_rows_ms"] = m * d * table.element_size() / COPY_CEILING_BYTES_PER_S * 1e3
    g = dev.gather_rows(table, at)                                       # not timed: the parent's forward made this copy
    out["e_weight_gradient"] = compare(lambda: dev.linear_wgrad_rows(table, idx, dz_buf), lambda: dev.linear_wgrad(g, dz_buf), args, f"(e) {tag}",
                                       names)
    return out


ONE_PASS_SHAPES = ((100, 47), (200, 3))


def one_pass_table(n_rows, m, d, c, dtype, args):
    """leg (f): the one-pass step against the K21 step on the batch matrix and against the K22 in-place step on the stored rows"""
    dev_ = torch.device("cuda", 0)
    gen = torch.Generator(device=dev_).manual_seed(args.seed)
    table = dev.alloc_rows(n_rows, d, dev_, dtype=dtype)
    table.copy_(torch.randn((n_rows, d), generator=gen, device=dev_))
    idx = None if m == n_rows else torch.randint(0, n_rows, (m,), generator=gen, device=dev_)
    at = torch.arange(n_rows, device=dev_) if idx is None else idx
    dense = idx is None and dtype == torch.float32                     # the table is the batch matrix: nothing is gathered
    lin = torch.nn.Linear(d, c).to(dev_)
    w, b = lin.weight, lin.bias
    wd, bd = w.detach(), b.detach()
    y = torch.randint(0, c, (m,), generator=gen, device=dev_)
    g = table if dense else dev.gather_rows(table, at)
    dw, db, loss, pred = dev.linear_step_rows(table, idx, wd, bd, y, 1.0, row_loss=True, pred=True)
    dz = dev.linear_class_loss(g, wd, bd, y, 1.0, dz=True)[0]
    check_sample(g, wd, bd, y, dz, loss, pred)
    want = dz.double().t() @ torch.cat((g.double(), torch.ones((m, 1), dtype=torch.float64, device=dev_)), 1)
    have = torch.cat((dw, db[:, None]), 1).double()
    assert float((have - want).abs().max()) <= 1e-4 * float(want.abs().max()), "dW / db of the one-pass step are off float64"
    del g, dz, want
    tag = f"n_rows={n_rows} m={m} d={d} C={c} {str(dtype).replace('torch.', '')}"
    out = {"n_rows": n_rows, "m": m, "index": "none" if idx is None else "random", "d": d, "c": c, "dtype": str(dtype).replace("torch.", "")}
    rows = range(n_rows) if idx is None else idx

    def step(one_pass, in_place):
        lin.zero_grad(set_to_none=True)
        if in_place:
            loss_ = cl.linear_cross_entropy(table, w, b, y, check=False, rows=rows, one_pass=one_pass)
        else:
            loss_ = cl.linear_cross_entropy(table if dense else dev.gather_rows(table, at), w, b, y, check=False, one_pass=one_pass)
        loss_.backward()
        return loss_

    out["f1_step_on_the_batch_matrix"] = compare(lambda: step(True, False), lambda: step(False, False), args, f"(f1) {tag}", ("one_pass", "k21"))
    out["f2_step_on_stored_rows"] = compare(lambda: step(True, True), lambda: step(False, True), args, f"(f2) {tag}", ("one_pass", "k22"))
    out["d_one_read_of_the_rows_ms"] = m * d * table.element_size() / COPY_CEILING_BYTES_PER_S * 1e3
    return out


def main_one_pass(args):
    sizes = sorted({int(n) for n in args.rows.split(",")})
    n_rows = sizes[-1]
    results = [one_pass_table(n_rows, m, d, c, dtype, args) for dtype in (torch.float32, torch.bfloat16) for m in sizes for d, c in ONE_PASS_SHAPES]
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "copy_ceiling_bytes_per_s": COPY_CEILING_BYTES_PER_S,
           "protocol": "legs interleaved in one process, HIP events, median (min - max); loss and pred of 64 sampled rows and dW, db checked "
                       "against float64 first; a step is linear_cross_entropy + backward, the gather is part of both candidates of (f1)",
           "expectation": "m d e bytes of features against 2 m d 4 + 2 m C 4 (plus the gather): a lower time than the K21 step and than the "
                          "K22 in-place step",
           "not_measured": ["hardware counters (LDS bank conflicts, FETCH bytes)", "a sweep of loss_blocks", "mini-batches below 196 615 rows",
                            "the step inside node_classification end to end"],
           "results": results}
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "linear_head_step.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def main_in_place(args):
    sizes = sorted({int(n) for n in args.rows.split(",")})
    n_rows = sizes[-1]
    results = [one_table(n_rows, m, d, c, dtype, args) for dtype in (torch.float32, torch.bfloat16) for m in sizes for d, c in SHAPES
               if not (dtype == torch.float32 and m == n_rows)]
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "copy_ceiling_bytes_per_s": COPY_CEILING_BYTES_PER_S,
           "protocol": "legs interleaved in one process, HIP events, median (min - max); in-place outputs of 64 sampled rows checked against "
                       "float64 first; the comparison point is gather_rows + K21 of the same process, its index on the device",
           "expectation": "fewer bytes (2 m d e against m d e + 12 m d), hence a lower time in (b) and (c)",
           "not_measured": ["hardware counters (FETCH bytes, L2 hit rates of the random rows)", "sorted or clustered index lists",
                            "mini-batches below 196 615 rows", "C > 172",
                            "host index lists (their upload is the same on both sides; for a bfloat16 full pass the parent uploads N indices per "
                            "call, which the in-place path does not)",
                            "a float32 table without an index (K21's own instance)", "the in-place step inside node_classification end to end"],
           "results": results}
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "linear_head_rows.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-place", action="store_true", help="measure the head on stored rows (K22) against gather_rows + K21")
    ap.add_argument("--one-pass", action="store_true", help="measure the one-pass step (K23) against the K21 step and the K22 in-place step")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", default=",".join(str(n) for n in ROWS))
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    _lib.require_gpu()
    torch.cuda.set_device(0)
    if args.in_place:
        return main_in_place(args)
    if args.one_pass:
        return main_one_pass(args)
    results = [one_shape(int(n), d, c, args) for n in args.rows.split(",") for d, c in SHAPES]
    doc = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "copy_ceiling_bytes_per_s": COPY_CEILING_BYTES_PER_S,
           "protocol": "legs interleaved in one process, HIP events, median (min - max); fused outputs of 64 sampled rows checked against float64 first",
           "not_measured": ["hardware counters (LDS bank conflicts, FETCH bytes)", "mini-batch steps below 196 615 rows", "C > 172"],
           "results": results}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

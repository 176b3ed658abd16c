"""Call trace of the device layer: which libsgl_hip entry points sgl_amd.device reaches, with which arguments.

    python tools/trace_calls.py > trace.jsonl

`device.lib` is replaced by a function that returns a recording proxy of the real library; a fixed list of valid calls then runs on the
GPU and every library call becomes one JSON line: the symbol, every scalar verbatim, every int64 array verbatim (the leading
dimensions), every address as null / non-null plus its value modulo 16, pointer arrays likewise.  The proof of a refactor of the
binding layer: copy this file into a checkout of the commit before, run it at both, and `cmp` the two outputs -- the pad, the
pitch and the vector path a call takes are all arguments.  Only names that the package has had since the bfloat16 aggregators are
used.  Every case is a valid call; the shapes are the smallest at which a path can flip, so the run takes seconds."""
import ctypes
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgl_amd import _lib, config                                              # noqa: E402
from sgl_amd import device as dev                                             # noqa: E402
from sgl_amd.operators.graph_op.laplacian_graph_op import LaplacianGraphOp    # noqa: E402

CUDA = torch.device("cuda", 0)
LINES = [0]


def _addr(v):
    return "null" if not v else f"addr%16={int(v) % 16}"


def describe(a):
    if a is None:
        return "null"
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, int):
        return a
    if isinstance(a, float):
        return repr(a)                                   # nan / inf stay readable, and JSON stays strict
    if isinstance(a, bytes):
        return a.decode()
    if isinstance(a, ctypes.Array):
        if a._type_ is ctypes.c_void_p:
            return [_addr(v) for v in a]
        return [int(v) for v in a]
    if isinstance(a, ctypes.c_void_p):
        return _addr(a.value)
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    return type(a).__name__                              # byref(...) of an output argument


class Recorder:
    """the real library, every sgl_* call written down before it is made"""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("sgl_") or name.endswith("_destroy"):     # (a handle is released whenever its owner is collected)
            return fn

        def call(*args):
            LINES[0] += 1
            print(json.dumps({"call": name, "args": [describe(a) for a in args]}), flush=False)
            return fn(*args)
        return call


def case(tag):
    print(json.dumps({"case": tag}))


# ---- hop lists ------------------------------------------------------------------------------------------------------------------
def rows(n, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    t = dev.alloc_rows(n, d, CUDA, dtype=dtype)
    t.copy_(torch.randn((n, d), generator=g))
    return t


def hop_lists(n, d, H):
    f32, bf16 = torch.float32, torch.bfloat16
    yield "f32", [rows(n, d, f32, h) for h in range(H)]
    yield "bf16", [rows(n, d, bf16, h) for h in range(H)]
    yield "mixed", [rows(n, d, bf16 if h % 2 else f32, h) for h in range(H)]
    slab = torch.randn((n, H * d), generator=torch.Generator().manual_seed(7)).to(CUDA)
    yield "slab", [slab[:, h * d:(h + 1) * d] for h in range(H)]
    yield "dense", [torch.randn((n, d), generator=torch.Generator().manual_seed(h)).to(CUDA) for h in range(H)]


def param(*shape, seed=3):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(CUDA).requires_grad_()


REFUSED = [0]


def run(label, fn):
    """one call of the list; a refusal by the library (an error code, nothing launched) is written down and counted: the list is
    meant to hold none"""
    try:
        return fn()
    except _lib.SglHipError as e:
        REFUSED[0] += 1
        print(json.dumps({"refused": label, "by": str(e).split(" failed")[0]}))


def backward(label, fn):
    def go():
        out = fn()
        (out[0].sum() + out[1].sum() if isinstance(out, tuple) else out.sum()).backward()
    run(label, go)


def aggregators(n, d, H, form, feats):
    R = _lib
    for op in (R.SGL_REDUCE_SUM, R.SGL_REDUCE_MEAN, R.SGL_REDUCE_MAX, R.SGL_REDUCE_MIN):
        run("hop_reduce", lambda: dev.hop_reduce(op, feats))
    run("hop_reduce wsum", lambda: dev.hop_reduce(R.SGL_REDUCE_WSUM, feats, torch.linspace(0.5, 1.5, H)))
    run("hop_concat", lambda: dev.hop_concat(feats))
    run("hop_concat f32", lambda: dev.hop_concat(feats, out_dtype=torch.float32))
    if form == "bf16":
        run("hop_concat bf16", lambda: dev.hop_concat(feats, out_dtype=torch.bfloat16))
    if H <= 16:
        run("hop_lincomb", lambda: dev.hop_lincomb(feats, torch.linspace(-1.0, 1.0, 2 * H).view(2, H)))
    run("nafs_aggregate", lambda: dev.nafs_aggregate(feats, return_weights=True))
    packed = form in ("slab", "dense") and d % 4 != 0         # rows that are not 16-byte vectors
    if d <= 512 and not packed:                               # (what sgl_nafs_prefix_f32 takes)
        run("nafs_prefix", lambda: dev.nafs_prefix(feats, sorted({0, H // 2, H - 1})))
    wide = dev.widen_hops(feats)                      # what MessageOp.aggregate hands to everything without a bfloat16 form

    def hot():
        return [f.detach().requires_grad_() for f in wide]
    # A single row has the leading dimension d (device._ld; a packed one in the hop table too): where d is no multiple of 4 the
    # kernels that want 16-byte rows refuse it although gate_fusable / hop_colsum let a single row pass.  Not asked for here.
    lone = n == 1 and d % 4 != 0 and packed
    if not (n == 1 and d % 4 and dev.gate_fusable(wide)):
        for name, fn, shape in (("hop_gate", dev.hop_gate, (d,)), ("hop_recursive", dev.hop_recursive, (1, 2 * d))):
            with torch.no_grad():
                run(name + " inference, weights", lambda: fn(wide, param(*shape), param(1), return_weights=True))
                run(name + " inference", lambda: fn(wide, param(*shape), param(1)))
            if lone:
                continue
            backward(name + " training", lambda: fn(wide, param(*shape), param(1), return_weights=True)[0])
            backward(name + " training, hop gradients", lambda: fn(hot(), param(*shape), param(1)))
    if not lone:
        backward("hop_scores", lambda: dev.hop_scores(wide, param(d)))
    if dev.gate_fusable(wide) and not lone:
        backward("hop_scores2", lambda: dev.hop_scores2(wide, param(d), param(H, d), (1 << H) - 2 if H > 1 else 1, 0, H))
    backward("hop_wsum1d", lambda: dev.hop_wsum1d(wide, param(H)))
    backward("hop_wsum2d", lambda: dev.hop_wsum2d(wide, param(n, H)))
    backward("hop_wsum2d, hop gradients", lambda: dev.hop_wsum2d(hot(), param(n, H)))
    backward("hop_reduce_grad max", lambda: dev.hop_reduce_grad(R.SGL_REDUCE_MAX, hot()))
    if lone:
        return
    run("hop_colsum", lambda: dev.hop_colsum(wide, torch.ones((n, H), device=CUDA)))
    run("hop_colsum shared", lambda: dev.hop_colsum(wide, torch.ones(n, device=CUDA), shared=True))


def gathers(n, d, H, form, feats):
    for m in (0, 1, 5):
        host = [(3 * i) % n for i in range(m)]
        for idx in (host, torch.tensor(host, dtype=torch.int64, device=CUDA)):
            run("gather_hops", lambda: dev.gather_hops(feats, idx))
            run("gather_rows", lambda: dev.gather_rows(feats[0], idx))
            run("gather_rows, padded out", lambda: dev.gather_rows(feats[0], idx, out=dev.alloc_rows(m, d, CUDA)))
            run("gather_rows, dense out", lambda: dev.gather_rows(feats[0], idx, out=torch.empty((m, d), device=CUDA)))
    if form in ("f32", "slab", "dense"):
        src = torch.tensor([0, n - 1], device=CUDA)[:min(n, 2)]
        run("scatter_rows", lambda: dev.scatter_rows(feats[0], src, torch.arange(src.numel(), device=CUDA), dev.alloc_rows(3, d, CUDA)))
        run("column_signature", lambda: dev.column_signature(feats[0]))
        cap, dev.EDGE_DOT_MAX_EDGES = dev.EDGE_DOT_MAX_EDGES, 2
        try:
            for E in (0, 1, 5):
                e = [[i % n, (2 * i) % n] for i in range(E)]
                run("edge_dot", lambda: dev.edge_dot(feats[0], feats[-1], np.asarray(e, dtype=np.int64).reshape(E, 2)))
        finally:
            dev.EDGE_DOT_MAX_EDGES = cap


def graph(n=37):
    rng = np.random.default_rng(5)
    a = sp.random(n, n, density=0.15, random_state=rng, format="csr", dtype=np.float32)
    a = ((a + a.T) > 0).astype(np.float32).tocsr()
    a.setdiag(0)
    a.eliminate_zeros()
    return a.tocsr()


def graph_cases():
    adj = graph()
    n = adj.shape[0]
    rowptr = torch.from_numpy(adj.indptr.astype(np.int64)).to(CUDA)
    col = torch.from_numpy(adj.indices.astype(np.int32)).to(CUDA)
    val = torch.from_numpy(adj.data.astype(np.float32)).to(CUDA)
    for alpha in (None, 0.2, 1.0):
        case(f"normalize_adj alpha={alpha}")
        run("dev.normalize_adj", lambda: dev.normalize_adj(rowptr, col, val, n, 0.5, alpha))
        run("dev.normalize_adj", lambda: dev.normalize_adj(rowptr, col, val, n, 0.5, alpha, host_pow=False))
    rp, ci, va = dev.normalize_adj(rowptr, col, val, n, 0.5)
    csr = dev.DeviceCSR(rp, ci, va, (n, n))
    run("csr.info", lambda: csr.info())
    for d in (3, 4, 100, 147, 513):
        for dtype in (torch.float32, torch.bfloat16):
            case(f"spmm d={d} {dtype}")
            x = rows(n, d, dtype, 1)
            y = run("spmm", lambda: csr.spmm(x))
            run("csr.spmm", lambda: csr.spmm(dev.padded_parent(x), out=dev.padded_parent(y)))
            acc = dev.alloc_rows(n, d, CUDA)
            acc.zero_()
            for mode in ("sum", "wsum", "max", "min"):
                run("csr.spmm_acc", lambda: csr.spmm_acc(x, y, acc, w=0.5 if mode == "wsum" else 1.0,
                                                         divisor=1.0 if mode in ("max", "min") else 2.0, mode=mode))
            run("csr.spmm_chain", lambda: csr.spmm_chain(x, 3))
            run("csr.spmm_chain", lambda: csr.spmm_chain(dev.padded_parent(x), 2))
        case(f"spmm_axpb_clamp d={d}")
        x = rows(n, d, torch.float32, 2)
        run("csr.spmm_axpb_clamp", lambda: csr.spmm_axpb_clamp(x, 0.9, res=rows(n, d, torch.float32, 3), lo=0.0, hi=1.0))
        run("csr.spmm_axpb_clamp", lambda: csr.spmm_axpb_clamp(x, 0.9))
    config.share_hops = False
    for hop_dtype in ("float32", "bfloat16"):
        for d in (3, 100, 147):
            feat = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32)
            op = LaplacianGraphOp(3, r=0.5, hop_dtype=hop_dtype)
            case(f"propagate {hop_dtype} d={d}")
            run("op.propagate", lambda: op.propagate(adj, feat))
            for kind in ("last", "sum", "mean", "max", "min", "wsum"):
                for start, end in ((0, None), (1, 3), (3, 4)):
                    case(f"propagate_reduce {hop_dtype} d={d} {kind} [{start}, {end})")
                    width = (4 if end is None else end) - start
                    run("propagate_reduce", lambda: op.propagate_reduce(
                        adj, feat, kind, start=start, end=end, weights=[0.5 + 0.25 * i for i in range(width)] if kind == "wsum" else None))


def main():
    _lib.require_gpu()
    real = _lib.lib()
    proxy = Recorder(real)
    dev.lib = lambda: proxy
    for n in (1, 2, 37):
        for d in (3, 4, 100, 147, 513):
            for H in (1, 3, 17):
                for form, feats in hop_lists(n, d, H):
                    case(f"aggregators n={n} d={d} H={H} {form}")
                    aggregators(n, d, H, form, feats)
                    case(f"gathers n={n} d={d} H={H} {form}")
                    gathers(n, d, H, form, feats)
    for n in (2, 37):
        case(f"hop_colsum n={n} d=1025")
        feats = [rows(n, 1025, torch.float32, h) for h in range(3)]
        dev.hop_colsum(feats, torch.ones((n, 3), device=CUDA))
    graph_cases()
    torch.cuda.synchronize()
    sys.stdout.flush()
    sys.stderr.write(f"trace_calls: {LINES[0]} library calls, {REFUSED[0]} refused\n")


if __name__ == "__main__":
    main()

"""Every entry point that takes a row width, on rows far wider than the project's 100 - 500 columns, on a real MI355X: run with
`-m gpu`.

The C ABI accepts d up to SGL_MAX_WIDTH = 2^31 - 1 - 4096 at practically every entry point, and the code dispatches on the width: the
SpMM cuts d into column slices of 256 lanes and reuses one split-row workspace from slice to slice, the concat has five routes chosen
by H d, the row-wise aggregators and the loss kernels leave their register layouts for streaming kernels, every flat-index kernel
divides by d.  wide_common.py holds the case table (proven complete against the headers by test_wide_cpu.py), the widths -- 4 100,
65 537, 65 540, 65 544, 1 048 580, each beyond a threshold -- and the launch arithmetic; here every case runs.

Inputs are padded views whose pad columns hold NaN in one run and 1e30 in the next; outputs are pre-filled with a sentinel NaN that
no kernel produces, in a buffer that continues GUARD_ROWS rows beyond the last row: after every call no sentinel may be left inside
the rows and everything around them must still hold it.

Comparisons.  Bit for bit wherever the entry point's own small test is bit-exact (strict-order SpMM against oracle_spmm, the fast
order against the slot model, bfloat16 against the bf16 model, copies, max / min, select_bwd, the bf16 aggregators against widening
first, the column signature against its definition; sgl_hop_lincomb_f32 with weights that are powers of two, for which one fma is one
float32 addition of exact products).  Everything that sums along the row through oracle.truth_report with its defaults -- at most
twice as far from the float64 truth as numpy's float32 evaluation of the same formula, floor 16 float32 roundings -- and the measured
errors are printed per case ("[wide err]"): nobody had measured them at 10^5 - 10^6 terms.  No tolerance is chosen in this file;
three bars are BORROWED, each with the comparison it belongs to: parity 1e-5 for accumulate = 1 on fast-order handles (the fast order
continues no chain from Y, so there is no bit model: test_gpu_far_offsets.test_spmm_f32; the per-slice offset of Y is pinned bit for
bit by the strict handles and by accumulate = 0), parity 2e-5 for the NAFS prefix sweep at its limit (test_gpu_agg_variants'
prefix_case) and 2e-6 of sum |w x| for the column sums (test_hop_colsum_is_the_weight_gradient_of_the_row_dots).

Entry points go through their device.py wrapper where the wrapper can write into a caller's buffer (DeviceCSR.*, gather_rows,
scatter_rows, column_signature, edge_dot, edge_loss_grad, class_loss_grad, cluster_loss_grad, kmeans_assign); the wrappers that
allocate their own output (hop_reduce, hop_concat, nafs_aggregate, ...) cannot take a sentinel-filled, guarded one, so those entry
points run through device._call, the one call path under every wrapper, and sgl_synth_features through probe_lib() on a buffer with
a guard band (synthetic.hashed_features_torch allocates).

The last test compares the record of what ran with the table, so a family that silently loses a case fails."""
import collections
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import class_loss_common as clc
import cluster_loss_common as cll
import edge_loss_common as elc
import kmeans_common as kc
import oracle
import oracle.torch_combine as tc
import wide_common as wc
from agg_rows_common import BIAS, gate_reference, recursive_step_by_step, reduce_statement, rne, same_bits32, sig_mix, t32, t64, vector
from inputs import hash_matrix
from sgl_amd import _lib, synthetic
from sgl_amd import device as dev
from sgl_amd.tricks.link_prediction import EdgePlan
from spmm_order_common import default_long_row_nnz, dispatch, parse_template_args

pytestmark = pytest.mark.gpu

NAN = float("nan")
POISONS = (NAN, 1e30)
SENT = wc.SENTINEL32
OPS = {"sum": _lib.SGL_REDUCE_SUM, "mean": _lib.SGL_REDUCE_MEAN, "max": _lib.SGL_REDUCE_MAX, "min": _lib.SGL_REDUCE_MIN,
       "wsum": _lib.SGL_REDUCE_WSUM}
RAN = collections.defaultdict(set)               # entry point -> {(width, layout)}: compared with the table by the last test


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def ints(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def sentinel_of(t):
    return SENT & 0xFFFF if t.element_size() == 2 else SENT


def place(n, d, layout):
    """(pitch, first column) of an [n, d] view: "padded" 16-byte rows on a pitch that is a multiple of 8 with at least 8 pad
    columns; "offset" the same pitch, the view one element in (rows aligned to their element only); "odd" an odd pitch"""
    if layout == "odd":
        return d + 1 + d % 2, 0
    return dev.round_up(d, 8) + 8, {"padded": 0, "offset": 1}[layout]


def inp(host, cuda, layout="padded", poison=NAN):
    """host values as a device view whose surroundings -- the pad columns of its own pitch -- hold `poison`"""
    host = host if torch.is_tensor(host) else torch.from_numpy(np.ascontiguousarray(host))
    n, d = host.shape
    pitch, c0 = place(n, d, layout)
    parent = torch.full((n, pitch), poison, dtype=host.dtype, device=cuda)
    view = parent[:, c0:c0 + d]
    view.copy_(host)
    return view


class Out:
    """an [n, d] output view of a sentinel-filled buffer with GUARD_ROWS more rows; written(): the kernel left no sentinel in
    columns [0, cols) of the rows (cols = d, or d + pad_cols: then the pad holds zeros) and nothing else was touched"""

    def __init__(self, n, d, cuda, layout="padded", dtype=torch.float32):
        self.n, self.d = n, d
        pitch, self.c0 = place(n, d, layout)
        self.parent = torch.empty((n + wc.GUARD_ROWS, pitch), dtype=dtype, device=cuda)
        ints(self.parent).fill_(sentinel_of(self.parent))
        self.t = self.parent[:n, self.c0:self.c0 + d]

    def written(self, pad=0):
        s, w = sentinel_of(self.parent), ints(self.parent).clone()
        mine = w[:self.n, self.c0:self.c0 + self.d + pad]
        left = int((mine == s).sum())
        zeros = pad == 0 or not bool(mine[:, self.d:].any())
        mine.fill_(s)
        return left == 0 and zeros and bool((w == s).all())


def out_vec(n, cuda, dtype=torch.float32, fill=None):
    """a length-n vector inside a longer sentinel vector: (view, check)"""
    whole = torch.empty(n + 8, dtype=dtype, device=cuda)
    if dtype == torch.float32:
        whole.view(torch.int32).fill_(SENT)
    else:
        whole.fill_(-7)
    view = whole[4:4 + n]

    def check():
        w = whole.clone()
        ok = not bool((w[4:4 + n].view(torch.int32) == SENT).any()) if dtype == torch.float32 else not bool((w[4:4 + n] == -7).any())
        w[4:4 + n] = w[0]
        return ok and bool((w.view(torch.int32) == SENT).all() if dtype == torch.float32 else (w == -7).all())
    return view, check


def ld(t):
    return t.stride(0)


def P(t):
    return None if t is None else _lib.ptr(t)


def call(name, *args):
    dev._call(None, name, *args)


def code(name, *args):
    rc = dev._call(None, name, *args, raw=True)
    return rc, _lib.last_error()


def ran(entry, width, layout="padded"):
    assert entry in wc.CASES, entry
    RAN[entry].add((width, layout))


def family_report(family):
    entries = [e for e, c in wc.CASES.items() if c.family == family]
    done = sum(len(RAN[e]) for e in entries)
    print(f"\n[wide {family}] {done} (entry point, width, layout) cases over {sum(1 for e in entries if RAN[e])} of {len(entries)} entry points")
    missing = [e for e in entries if not RAN[e]]
    assert not missing, missing


def truth(entry, what, n, W, got, ref32, t, cond=None):
    """the project's rule, figures printed before the assertion"""
    got = np.asarray(got)
    rep = oracle.truth_report(got, np.asarray(ref32), np.asarray(t), cond=None if cond is None else np.asarray(cond))
    print(f"[wide err] {entry} {what} n={n} W={W} hip={rep.get('err_got', NAN):.3e} ref32={rep.get('err_ref', NAN):.3e} bound={rep.get('bound', NAN):.3e}")
    assert np.isfinite(got).all() and rep["ok"], (entry, what, n, W, rep)


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


@contextlib.contextmanager
def tuned(**kw):
    saved = {k: _lib.get_tuning(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k, v in saved.items():
            _lib.set_tuning(k, v)


CONCAT_NAMES = ("hop_concat_rows_kernel", "hop_concat_lds_kernel", "hop_concat_any_kernel", "hop_concat_kernel")


def kernels_of(fn, names=CONCAT_NAMES):
    """[(kernel, template arguments or None)] of the kernels of `names` that ran inside fn(), as the profiler reports them
    (demangled `hop_concat_kernel<4>(...)` or mangled `...hop_concat_kernelILi4EEEv...`)"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = []
    for e in sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start):
        for kn in names:
            if kn in e.name:
                out.append((kn, parse_template_args(e.name[e.name.index(kn) + len(kn):])))
                break
    return out


def hop_weights(n_hops):
    return (np.float32(0.75) ** np.arange(n_hops, dtype=np.float32) * np.where(np.arange(n_hops) % 3 == 2, -1, 1)).astype(np.float32)


# ---- SpMM float32 ------------------------------------------------------------------------------------------------------------------
def handles(g, cuda):
    """{label: (DeviceCSR, strict)}: default and strict plans, each also on the row-permuted storage behind a row map"""
    def make(gr, strict):
        return dev.DeviceCSR(torch.from_numpy(gr.rowptr).to(cuda), torch.from_numpy(gr.col).to(cuda), torch.from_numpy(gr.val).to(cuda), (gr.n, gr.n),
                             strict=strict)
    pg, perm = wc.permuted(g)
    out = {}
    for strict in (False, True):
        tag = "strict" if strict else "fast"
        out[tag] = (make(g, strict), strict)
        out[tag + "+rowmap"] = (make(pg, strict).set_rowmap(torch.from_numpy(perm).to(cuda)), strict)
    for tag, (csr, strict) in out.items():
        info = csr.info()
        assert info["n_pieces"] == (0 if strict else 2) and info["n_long_rows"] == (0 if strict else 1), (tag, info)
    return out


def spmm_model(g, x, xd, yd, strict, bf16=False, acc=None):
    """the float32 sums of A x in the order of the kernels that run for these buffers: oracle_spmm (strict) or the slot model
    per column slice (spmm_order_common.dispatch gives the slices and their R), and the number of slices"""
    sl = dispatch("bf16" if bf16 else "f32", x.shape[1], ld(xd), ld(yd), xd.data_ptr(), yd.data_ptr(), strict, len(g.col) / g.n,
                  acc=None if acc is None else (ld(acc), acc.data_ptr()))
    if strict:
        return oracle.oracle_spmm(g.rowptr, g.col, g.val, x), len(sl)
    lr = default_long_row_nnz(len(g.col))
    y = np.empty((g.n, x.shape[1]), np.float32)
    for c0, dc, var in sl:
        y[:, c0:c0 + dc] = oracle.oracle_spmm_slots(g.rowptr, g.col, g.val, np.ascontiguousarray(x[:, c0:c0 + dc]), 64 // var[1], lr)
    return y, len(sl)


def acc_statement(mode, acc0, y, w, divisor):
    """sgl_spmm_acc's update in numpy float32 (the statement of test_gpu_far_offsets.py): add / rounded product then add /
    NaN-propagating max, min; then one true division"""
    with np.errstate(all="ignore"):
        if mode == 0:
            acc = acc0 + y
        elif mode == 1:
            acc = acc0 + np.float32(w) * y
        else:
            acc = (np.maximum if mode == 2 else np.minimum)(acc0, y)
        return (acc / np.float32(divisor)).astype(np.float32) if (mode < 2 and divisor != 1.0) else acc.astype(np.float32)


@pytest.mark.parametrize("W,layout", [(wc.W_CAP, "odd"), (wc.W_VEC, "padded")], ids=["4100-odd-pitch", "65540"])
def test_spmm_f32(cuda, W, layout):
    """sgl_spmm_f32 (both values of accumulate), _axpb_clamp (residual), _acc (every mode), _multi (two outputs), _chain (3 hops) and
    the captured chain graph on the split-row graph: 65 column slices of 1 024 at W = 65 540 (17 of 256 on the odd pitch), the
    residual / aggregate / replica pointers advanced per slice and the handle's one split-row workspace reused by every slice"""
    g = wc.graph()
    x, y0, res, acc0 = (hash_matrix(g.n, W, seed=s + W % 97) for s in (11, 12, 13, 14))
    for tag, (csr, strict) in handles(g, cuda).items():
        lay = f"{layout} {tag}"
        xd = inp(x, cuda, layout)
        # plain product, then accumulate into y0
        for accumulate in (False, True):
            o = Out(g.n, W, cuda, layout)
            if accumulate:
                o.t.copy_(torch.from_numpy(y0))
            csr.spmm(xd, out=o.t, accumulate=accumulate)
            ax, n_slices = spmm_model(g, x, xd, o.t, strict)
            assert n_slices == wc.spmm_slices(W, 1 if layout == "odd" else 4)
            want = ax if not accumulate else None
            got = o.t.cpu().numpy()
            if accumulate:                                                   # the kernel continues the fma chain from Y (strict order only is bit-defined)
                if strict:
                    assert np.array_equal(got, oracle.oracle_spmm(g.rowptr, g.col, g.val, x, out=y0.copy())), (lay, "accumulate")
                else:
                    assert oracle.parity_ok(got, oracle.oracle_spmm(g.rowptr, g.col, g.val, x, out=y0.copy()), 1e-5), (lay, "accumulate")
            else:
                assert same_bits32(got, want), (lay, int((got != want).sum()))
            assert o.written(), (lay, "spmm", accumulate)
        ran("sgl_spmm_f32", W, lay)
        # epilogue: residual and clamp
        o, rd = Out(g.n, W, cuda, layout), inp(res, cuda, layout, 1e30)
        csr.spmm_axpb_clamp(xd, 0.8, rd, -0.5, 0.75, out=o.t)
        want = np.clip((np.float32(0.8) * ax + res).astype(np.float32), np.float32(-0.5), np.float32(0.75))
        assert same_bits32(o.t.cpu().numpy(), want) and o.written(), (lay, "axpb_clamp")
        ran("sgl_spmm_axpb_clamp_f32", W, lay)
        # running aggregate, every mode
        for mode, w, divisor in ((0, 1.0, 1.0), (0, 1.0, 4.0), (1, -1.5, 3.0), (2, 1.0, 1.0), (3, 1.0, 1.0)):
            o, a = Out(g.n, W, cuda, layout), Out(g.n, W, cuda, layout)
            a.t.copy_(torch.from_numpy(acc0))
            call("sgl_spmm_acc_f32", csr._h, P(xd), ld(xd), P(o.t), ld(o.t), W, P(a.t), ld(a.t), w, mode, divisor)
            y = o.t.cpu().numpy()
            assert same_bits32(y, ax) and same_bits32(a.t.cpu().numpy(), acc_statement(mode, acc0, y, w, divisor)), (lay, "acc", mode)
            assert o.written() and a.written(), (lay, "acc", mode)
        ran("sgl_spmm_acc_f32", W, lay)
        # two outputs (a row-mapped handle refuses replicas: documented)
        o1, o2 = Out(g.n, W, cuda, layout), Out(g.n, W, cuda, layout)
        if "rowmap" in tag:
            with pytest.raises(_lib.SglHipError, match="row-mapped handle does not support replicas"):
                csr.spmm_multi(xd, [o1.t.data_ptr(), o2.t.data_ptr()], ld(o1.t))
        else:
            csr.spmm_multi(xd, [o1.t.data_ptr(), o2.t.data_ptr()], ld(o1.t))
            assert same_bits32(o1.t.cpu().numpy(), ax) and same_bits32(o2.t.cpu().numpy(), ax) and o1.written() and o2.written(), (lay, "multi")
            ran("sgl_spmm_multi_f32", W, lay)
        # chain of 3 hops, eagerly and as a captured graph
        outs = [Out(g.n, W, cuda, layout) for _ in range(3)]
        csr.spmm_chain(xd, 3, outs=[o.t for o in outs])
        prev, prev_d, hops = x, xd, []
        for k, o in enumerate(outs):
            want, _ = spmm_model(g, prev, prev_d, o.t, strict)
            got = o.t.cpu().numpy()
            assert same_bits32(got, want) and o.written(), (lay, "chain hop", k + 1, int((got != want).sum()))
            prev, prev_d = got, o.t
            hops.append(got)
        ran("sgl_spmm_chain_f32", W, lay)
        gouts = [Out(g.n, W, cuda, layout) for _ in range(3)]
        graph = csr.capture_chain(xd, [o.t for o in gouts])
        for o in gouts:
            ints(o.t).fill_(SENT)                                             # the capture ran the chain once: poison it again
        graph.replay()
        for k, o in enumerate(gouts):
            assert same_bits32(o.t.cpu().numpy(), hops[k]) and o.written(), (lay, "chain graph hop", k + 1)
        graph.close()
        ran("sgl_chain_graph_create", W, lay)
        # every entry point of the family refuses a wider row under its own name, before any launch (the outputs keep the sentinel)
        wide, q = wc.C["SGL_MAX_WIDTH"] + 1, Out(g.n, W, cuda, layout)
        one_y, one_ld, made = (ctypes.c_void_p * 1)(q.t.data_ptr()), (ctypes.c_int64 * 1)(ld(q.t)), ctypes.c_void_p()
        for entry, args in (("sgl_spmm_f32", (csr._h, P(xd), ld(xd), P(q.t), ld(q.t), wide, 0)),
                            ("sgl_spmm_axpb_clamp_f32", (csr._h, P(xd), ld(xd), P(q.t), ld(q.t), wide, 0.8, P(rd), ld(rd), -0.5, 0.75)),
                            ("sgl_spmm_acc_f32", (csr._h, P(xd), ld(xd), P(q.t), ld(q.t), wide, P(a.t), ld(a.t), 1.0, 0, 1.0)),
                            ("sgl_spmm_multi_f32", (csr._h, P(xd), ld(xd), 1, one_y, ld(q.t), wide, None)),
                            ("sgl_spmm_chain_f32", (csr._h, 1, P(xd), ld(xd), one_y, one_ld, wide)),
                            ("sgl_chain_graph_create", (ctypes.byref(made), csr._h, 1, P(xd), ld(xd), one_y, one_ld, wide))):
            rc, msg = code(entry, *args)
            assert rc == _lib.SGL_ERR_UNSUPPORTED and msg == f"{entry}: d={wide} is wider than SGL_MAX_WIDTH={wide - 1}", (entry, rc, msg)
        assert not made.value and bool((ints(q.parent) == SENT).all())
        csr.close()
    family_report("spmm")


def test_spmm_bf16(cuda):
    """sgl_spmm_bf16, sgl_spmm_chain_bf16 (3 hops) and sgl_spmm_acc_bf16 at W = 65 544: 33 slices of 2 048 columns in 8-element lanes;
    bit-equal to the bf16 model rne(float32 model(widened input))"""
    g, W = wc.graph(unit_rows=True), wc.W_BF16
    b0 = rne(hash_matrix(g.n, W, seed=5))
    acc0 = hash_matrix(g.n, W, seed=16)
    for tag, (csr, strict) in handles(g, cuda).items():
        xd = inp(b0, cuda)
        o = Out(g.n, W, cuda, dtype=torch.bfloat16)
        csr.spmm(xd, out=o.t)
        sums, n_slices = spmm_model(g, b0.float().numpy(), xd, o.t, strict, bf16=True)
        assert n_slices == wc.spmm_slices(W, 8)
        assert np.array_equal(bits16(o.t), bits16(rne(sums))) and o.written(), (tag, "spmm_bf16")
        ran("sgl_spmm_bf16", W, tag)
        outs = [Out(g.n, W, cuda, dtype=torch.bfloat16) for _ in range(3)]
        csr.spmm_chain(xd, 3, outs=[q.t for q in outs])
        prev, prev_d = b0, xd
        for k, q in enumerate(outs):
            sums, _ = spmm_model(g, prev.float().numpy(), prev_d, q.t, strict, bf16=True)
            assert np.array_equal(bits16(q.t), bits16(rne(sums))) and q.written(), (tag, "chain_bf16 hop", k + 1)
            prev, prev_d = q.t.cpu(), q.t
        ran("sgl_spmm_chain_bf16", W, tag)
        for mode, w, divisor in ((0, 1.0, 4.0), (1, -1.5, 1.0), (2, 1.0, 1.0), (3, 1.0, 1.0)):
            y, a = Out(g.n, W, cuda, dtype=torch.bfloat16), Out(g.n, W, cuda)
            a.t.copy_(torch.from_numpy(acc0))
            csr.spmm_acc(xd, y.t, a.t, w=w, divisor=divisor, mode={0: "sum", 1: "wsum", 2: "max", 3: "min"}[mode])
            sums, _ = spmm_model(g, b0.float().numpy(), xd, y.t, strict, bf16=True, acc=a.t)
            assert np.array_equal(bits16(y.t), bits16(rne(sums))) and y.written(), (tag, "acc_bf16 y", mode)
            assert same_bits32(a.t.cpu().numpy(), acc_statement(mode, acc0, y.t.float().cpu().numpy(), w, divisor)) and a.written(), (tag, "acc_bf16", mode)
        ran("sgl_spmm_acc_bf16", W, tag)
        wide, q = wc.C["SGL_MAX_WIDTH"] + 1, Out(g.n, W, cuda, dtype=torch.bfloat16)
        one_y, one_ld = (ctypes.c_void_p * 1)(q.t.data_ptr()), (ctypes.c_int64 * 1)(ld(q.t))
        for entry, args in (("sgl_spmm_bf16", (csr._h, P(xd), ld(xd), P(q.t), ld(q.t), wide)),
                            ("sgl_spmm_chain_bf16", (csr._h, 1, P(xd), ld(xd), one_y, one_ld, wide)),
                            ("sgl_spmm_acc_bf16", (csr._h, P(xd), ld(xd), P(q.t), ld(q.t), wide, P(a.t), ld(a.t), 1.0, 0, 1.0))):
            rc, msg = code(entry, *args)
            assert rc == _lib.SGL_ERR_UNSUPPORTED and msg == f"{entry}: d={wide} is wider than SGL_MAX_WIDTH={wide - 1}", (entry, rc, msg)
        assert bool((ints(q.parent) == sentinel_of(q.parent)).all())
        csr.close()
    family_report("spmm_bf16")


# ---- streaming aggregators ------------------------------------------------------------------------------------------------------------
def stream_cases():
    """(n, W, H, layout): every shape on padded views; the offset views (rows aligned to 4 bytes: one float per lane whatever d is)
    and the 17-hop list at the smallest width"""
    out = [(n, W, wc.H, "padded") for n, W in wc.shapes(wc.ALL4)]
    return out + [(3, wc.W_CAP, wc.H, "offset"), (3, wc.W_CAP, wc.H_MANY, "padded")]


def test_streaming_aggregators(cuda):
    """sgl_hop_reduce_f32 (5 ops), sgl_hop_wsum2d_f32 and its backward (dW and dX), sgl_hop_wsum1d_bwd_f32 (both routes: register
    partials for up to 16 hops of 16-byte rows, the scalar kernel otherwise), sgl_hop_select_bwd_f32 and sgl_hop_lincomb_f32"""
    for n, W, Hn, layout in stream_cases():
        hosts = wc.hops_host(n, W, Hn)
        for k, poison in enumerate(POISONS if (W == wc.W_CAP and Hn == wc.H) else POISONS[:1]):
            xs = [inp(h, cuda, layout, poison) for h in hosts]
            ptrs, lds = _lib.hop_arrays(xs)
            ctx = (n, W, Hn, layout, k)
            w1 = hop_weights(Hn)
            w1d = torch.from_numpy(w1).to(cuda)
            for kind, op in OPS.items():
                o = Out(n, W, cuda, layout)
                call("sgl_hop_reduce_f32", op, Hn, ptrs, lds, P(w1d) if kind == "wsum" else None, P(o.t), ld(o.t), n, W)
                assert same_bits32(o.t.cpu().numpy(), reduce_statement(kind, hosts, w1)) and o.written(), (ctx, kind)
            ran("sgl_hop_reduce_f32", W, f"{layout} H={Hn}")
            if Hn > 16:
                # the scalar route of the weight gradient by hop count
                g = hash_matrix(n, W, seed=7)
                gd, (dw, dw_ok) = inp(g, cuda, layout, poison), out_vec(Hn, cuda)
                scratch = torch.empty(int(_lib.lib().sgl_hop_wsum1d_bwd_scratch(Hn)), dtype=torch.float32, device=cuda)
                call("sgl_hop_wsum1d_bwd_f32", Hn, ptrs, lds, P(gd), ld(gd), P(dw), P(scratch), n, W)
                truth("sgl_hop_wsum1d_bwd_f32", "dw (17 hops: scalar route)", n, W, dw.cpu().numpy(),
                      np.array([(g * x).sum(dtype=np.float32) for x in hosts]), np.array([(g.astype(np.float64) * x).sum() for x in hosts]),
                      cond=np.array([(np.abs(g).astype(np.float64) * np.abs(x)).sum() for x in hosts]))
                assert dw_ok()
                ran("sgl_hop_wsum1d_bwd_f32", W, f"{layout} H={Hn}")
                continue
            w2 = oracle.softmax32(hash_matrix(n, Hn, seed=W % 89 + Hn), 1)
            g = hash_matrix(n, W, seed=5 * (W % 83) + 2)
            wd, gd = inp(w2, cuda, "offset", poison), inp(g, cuda, layout, poison)
            o = Out(n, W, cuda, layout)
            call("sgl_hop_wsum2d_f32", Hn, ptrs, lds, P(wd), ld(wd), P(o.t), ld(o.t), n, W)
            ref32 = np.zeros((n, W), np.float32)
            for h in range(Hn):
                ref32 = ref32 + w2[:, h:h + 1] * hosts[h]
            t = sum(w2[:, h:h + 1].astype(np.float64) * hosts[h] for h in range(Hn))
            truth("sgl_hop_wsum2d_f32", "out", n, W, o.t.cpu().numpy(), ref32, t)
            assert o.written(), ctx
            ran("sgl_hop_wsum2d_f32", W, layout)

            dwo, dxs = Out(n, Hn, cuda, "offset"), [Out(n, W, cuda, layout) for _ in hosts]
            dptrs, dlds = _lib.hop_arrays([q.t for q in dxs])
            call("sgl_hop_wsum2d_bwd_f32", Hn, ptrs, lds, P(wd), ld(wd), P(gd), ld(gd), P(dwo.t), ld(dwo.t), dptrs, dlds, n, W)
            g64 = g.astype(np.float64)
            truth("sgl_hop_wsum2d_bwd_f32", "dW", n, W, dwo.t.cpu().numpy(), np.stack([(g * x).sum(1, dtype=np.float32) for x in hosts], 1),
                  np.stack([(g64 * x).sum(1) for x in hosts], 1), cond=np.stack([(np.abs(g64) * np.abs(x)).sum(1) for x in hosts], 1))
            assert dwo.written() and all(np.array_equal(q.t.cpu().numpy(), w2[:, h:h + 1] * g) and q.written() for h, q in enumerate(dxs)), ctx
            ran("sgl_hop_wsum2d_bwd_f32", W, layout)

            dw, dw_ok = out_vec(Hn, cuda)
            scratch = torch.empty(int(_lib.lib().sgl_hop_wsum1d_bwd_scratch(Hn)), dtype=torch.float32, device=cuda)
            call("sgl_hop_wsum1d_bwd_f32", Hn, ptrs, lds, P(gd), ld(gd), P(dw), P(scratch), n, W)
            truth("sgl_hop_wsum1d_bwd_f32", "dw", n, W, dw.cpu().numpy(), np.array([(g * x).sum(dtype=np.float32) for x in hosts]),
                  np.array([(g64 * x).sum() for x in hosts]), cond=np.array([(np.abs(g64) * np.abs(x)).sum() for x in hosts]))
            assert dw_ok(), ctx
            ran("sgl_hop_wsum1d_bwd_f32", W, layout)

            base = [h.copy() for h in hosts]
            base[2][0, :W // 2] = base[0][0, :W // 2]                           # ties along half a row
            base[1][n - 1, W - 1] = np.nan
            bx = [inp(h, cuda, layout, poison) for h in base]
            bptrs, blds = _lib.hop_arrays(bx)
            for op, name in ((_lib.SGL_REDUCE_MAX, "max"), (_lib.SGL_REDUCE_MIN, "min")):
                dxs = [Out(n, W, cuda, layout) for _ in base]
                dptrs, dlds = _lib.hop_arrays([q.t for q in dxs])
                call("sgl_hop_select_bwd_f32", op, Hn, bptrs, blds, P(gd), ld(gd), dptrs, dlds, n, W)
                leaves = [torch.from_numpy(x.copy()).to(cuda).requires_grad_(True) for x in base]
                getattr(torch.stack(leaves, 0), name)(0)[0].backward(torch.from_numpy(g).to(cuda))
                assert all(torch.equal(q.t, leaves[h].grad) and q.written() for h, q in enumerate(dxs)), (ctx, name)
            ran("sgl_hop_select_bwd_f32", W, layout)

            # weights that are powers of two (and one zero): every product is exact, so one fma is one float32 addition of it
            wl = np.array([[0.5, -2.0, 0.25], [0.0, 1.0, -0.125]], dtype=np.float32)
            wld = torch.from_numpy(wl).to(cuda)
            outs = [Out(n, W, cuda, layout) for _ in wl]
            optrs, olds = _lib.hop_arrays([q.t for q in outs])
            call("sgl_hop_lincomb_f32", Hn, ptrs, lds, len(wl), optrs, olds, P(wld), Hn, n, W)
            for kk, q in enumerate(outs):
                want = np.zeros((n, W), np.float32)
                for j in range(Hn):
                    if wl[kk, j] != 0:
                        want = want + wl[kk, j] * hosts[j]
                assert same_bits32(q.t.cpu().numpy(), want) and q.written(), (ctx, "lincomb", kk)
            ran("sgl_hop_lincomb_f32", W, layout)
    family_report("stream")


# ---- concat ---------------------------------------------------------------------------------------------------------------------------
def concat_case(cuda, n, d, Hn, layout, pad, lds):
    hosts = wc.hops_host(n, d, Hn)
    xs = [inp(h, cuda, layout) for h in hosts]
    ptrs, plds = _lib.hop_arrays(xs)
    width = Hn * d
    o = Out(n, width + pad, cuda, layout)                                     # the view holds the row and its declared pad
    aligned = layout == "padded"
    route = wc.concat_route(Hn, d, pad, aligned, lds)

    def launch():
        if pad:
            call("sgl_hop_concat_padded_f32", Hn, ptrs, plds, P(o.t), ld(o.t), pad, n, d)
        else:
            call("sgl_hop_concat_f32", Hn, ptrs, plds, P(o.t), ld(o.t), n, d)
    with tuned(concat_lds=lds):
        seen = kernels_of(launch)
    name, arg = wc.CONCAT_KERNELS[route]
    assert len(seen) == 1 and seen[0][0] == name and (arg is None or seen[0][1] == [arg]), (seen, route, (n, d, Hn, layout, pad, lds))
    got = o.t.cpu().numpy()
    assert np.array_equal(got[:, :width].view(np.uint32), np.hstack(hosts).view(np.uint32)), (n, d, Hn, layout, pad, lds, route)
    assert not got[:, width:].view(np.uint32).any() and o.written(), (n, d, Hn, layout, pad, lds, route)
    return route


def test_concat_routes(cuda):
    """sgl_hop_concat_f32 / _padded_f32, bit-equal to hstack, and the kernel that ran is the one the restated launcher names: the
    16-byte copy (d % 4 == 0), the tile kernel and the funnel kernel beyond kConcatRowCap (concat_lds = 1 / 3 / 0: the whole-row kernel
    is legal nowhere at these widths, so 3 falls back to the tiles), the float-by-float copy behind offset views"""
    routes = collections.Counter()
    for n, W in wc.shapes(wc.ALL4):
        for layout in ("padded", "offset"):
            for pad in ((0, (-wc.H * W) % 4 + 4) if layout == "padded" else (0,)):
                for lds in ((0, 1, 3) if (W == wc.W_ODD or (W == wc.W_CAP and n == 9)) else (1,)):
                    routes[concat_case(cuda, n, W, wc.H, layout, pad, lds)] += 1
                    ran("sgl_hop_concat_padded_f32" if pad else "sgl_hop_concat_f32", W, f"{layout} lds={lds}")
    # the tile and the funnel kernel on ONE row and on a partial row block (3 of 8), padded and not; the odd-pitch layout (copy1)
    for n in (1, 3):
        for lds in (1, 0):
            for pad in (0, (-wc.H * wc.W_ODD) % 4 + 4):
                routes[concat_case(cuda, n, wc.W_ODD, wc.H, "padded", pad, lds)] += 1
                ran("sgl_hop_concat_padded_f32" if pad else "sgl_hop_concat_f32", wc.W_ODD, f"padded n={n} lds={lds}")
    routes[concat_case(cuda, 3, wc.W_CAP, wc.H, "odd", 0, 1)] += 1
    ran("sgl_hop_concat_f32", wc.W_CAP, "odd pitch")
    # 17 hops at the smallest width; one column more makes the row unaligned for the 16-byte copy: tiles, funnel
    for d, lds in ((wc.W_CAP, 1), (wc.W_CAP + 1, 1), (wc.W_CAP + 1, 0), (wc.W_CAP + 1, 3)):
        routes[concat_case(cuda, 9, d, wc.H_MANY, "padded", (-wc.H_MANY * d) % 4 + 4, lds)] += 1
        ran("sgl_hop_concat_padded_f32", wc.W_CAP, f"padded H={wc.H_MANY} d={d} lds={lds}")
    print(f"\n[wide concat] routes taken: {dict(routes)}")
    assert set(routes) == {"copy4", "copy1", "lds", "any"}                     # "rows" is for rows of up to 4 096 floats: not legal here
    family_report("concat")


def test_concat_beyond_2_31_columns(cuda):
    """H = 64 hops of d = 33 554 433 columns, n = 1: H d = 2^31 + 64, d % 4 = 1 -- the rows hop_concat_kernel<1> is the fallback for,
    where its flat remainder `rem` leaves 32 bits (it formed the hop and the column from (int)rem: the hop went negative and
    hx.p[h] was read outside the argument struct; fixed before this case first ran).  All 64 hop pointers name one 134 MB row made
    by sgl_synth_features; the 8.6 GB output is checked on the device: sampled columns of every hop segment -- its first and last,
    both sides of every power of two from 2^15 -- against the generator recomputed column by column, and the count of sentinels left."""
    Hn, d, n = wc.HUGE["H"], wc.HUGE["d"], wc.HUGE["n"]
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < wc.HUGE_NEEDS:
        pytest.skip(f"the 2^31-column concat needs {wc.HUGE_NEEDS / 2 ** 30:.0f} GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    row = torch.empty((1, d), dtype=torch.float32, device=cuda)
    _lib.check_probe(_lib.probe_lib().sgl_synth_features(ctypes.c_uint64(77), 0, 1, d, d, _lib.ptr(row), _lib.current_stream_ptr()), "sgl_synth_features")
    width = Hn * d
    guard = 1 << 20
    buf = torch.empty(width + guard, dtype=torch.float32, device=cuda)
    step = 1 << 28
    for lo in range(0, buf.numel(), step):
        buf[lo:lo + step].view(torch.int32).fill_(SENT)
    out = buf[:width].view(1, width)
    ptrs = (ctypes.c_void_p * Hn)(*[row.data_ptr()] * Hn)
    lds = (ctypes.c_int64 * Hn)(*[d] * Hn)
    seen = kernels_of(lambda: call("sgl_hop_concat_f32", Hn, ptrs, lds, P(out), width, n, d))
    assert len(seen) == 1 and seen[0] == ("hop_concat_kernel", [1]), seen
    pos, hop, src = wc.concat_samples(Hn, d, lambda h: wc.sample_columns(d, 96, seed=h))
    want = wc.hashed_features_at(77, 0, src)
    got = buf[torch.from_numpy(pos).to(cuda)].cpu().numpy()
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad.size, [(int(hop[b]), int(src[b])) for b in bad[:8]])
    left = sum(int((buf[lo:min(lo + step, width)].view(torch.int32) == SENT).sum()) for lo in range(0, width, step))
    assert left == 0, left
    assert bool((buf[width:].view(torch.int32) == SENT).all())                  # the guard band behind the row
    # every segment is the row itself: the whole output, compared on the device segment by segment
    assert all(torch.equal(buf[h * d:(h + 1) * d], row[0]) for h in range(Hn))
    print(f"\n[wide concat 2^31] H d = {width} columns ({width * 4 / 1e9:.1f} GB), {len(pos)} sampled places and all {Hn} segments equal; {free / 2 ** 30:.1f} GiB were free")
    ran("sgl_hop_concat_f32", d, "H=64 n=1")
    del buf, out, row
    torch.cuda.empty_cache()


# ---- bfloat16 aggregators -----------------------------------------------------------------------------------------------------------------
def test_aggregators_bf16(cuda):
    """sgl_hop_reduce_bf16_f32 (5 ops), sgl_hop_concat_bf16 and sgl_hop_concat_bf16_f32: bit-equal to the float32 statement over the
    widened hops and to "widen first, then the float32 entry point"; 8-element lanes at 65 544, narrower ones at 4 100 (4) and 65 537 (1)"""
    for n, W in wc.shapes((wc.W_CAP, wc.W_ODD, wc.W_BF16)):
        for layout in (("padded", "offset") if W == wc.W_CAP else ("padded",)):
            hosts16 = [rne(h) for h in wc.hops_host(n, W, wc.H, seed=2)]
            wide = [h.float().numpy() for h in hosts16]
            xs = [inp(h, cuda, layout) for h in hosts16]
            ptrs, lds = _lib.hop_arrays(xs)
            widened = [inp(w, cuda) for w in wide]
            w1 = hop_weights(wc.H)
            w1d = torch.from_numpy(w1).to(cuda)
            ctx = (n, W, layout)
            for kind, op in OPS.items():
                o = Out(n, W, cuda, layout)
                call("sgl_hop_reduce_bf16_f32", op, wc.H, ptrs, lds, P(w1d) if kind == "wsum" else None, P(o.t), ld(o.t), 0, n, W)
                y = o.t.cpu().numpy()
                assert same_bits32(y, reduce_statement(kind, wide, w1)) and o.written(), (ctx, kind)
                assert same_bits32(y, dev.hop_reduce(op, widened, w1d if kind == "wsum" else None).cpu().numpy()), (ctx, kind)
            pad = 8 - W % 8 if layout == "padded" else 0
            o = Out(n, W + pad, cuda, layout)
            call("sgl_hop_reduce_bf16_f32", OPS["sum"], wc.H, ptrs, lds, None, P(o.t), ld(o.t), pad, n, W)
            y = o.t.cpu().numpy()
            assert same_bits32(y[:, :W], reduce_statement("sum", wide, w1)) and not y[:, W:].view(np.uint32).any() and o.written(), (ctx, "padded sum")
            ran("sgl_hop_reduce_bf16_f32", W, layout)
            o16, o32 = Out(n, wc.H * W, cuda, layout, dtype=torch.bfloat16), Out(n, wc.H * W, cuda, layout)
            call("sgl_hop_concat_bf16", wc.H, ptrs, lds, P(o16.t), ld(o16.t), 0, n, W)
            call("sgl_hop_concat_bf16_f32", wc.H, ptrs, lds, P(o32.t), ld(o32.t), 0, n, W)
            assert np.array_equal(bits16(o16.t), bits16(torch.cat(hosts16, dim=1))) and o16.written(), ctx
            assert np.array_equal(o32.t.cpu().numpy().view(np.uint32), np.hstack(wide).view(np.uint32)) and o32.written(), ctx
            if layout == "padded":                                             # ... and with declared pad columns: zeros
                cp = (-wc.H * W) % 8 + 8
                p16, p32 = Out(n, wc.H * W + cp, cuda, dtype=torch.bfloat16), Out(n, wc.H * W + cp, cuda)
                call("sgl_hop_concat_bf16", wc.H, ptrs, lds, P(p16.t), ld(p16.t), cp, n, W)
                call("sgl_hop_concat_bf16_f32", wc.H, ptrs, lds, P(p32.t), ld(p32.t), cp, n, W)
                g16, g32 = bits16(p16.t), p32.t.cpu().numpy().view(np.uint32)
                assert np.array_equal(g16[:, :wc.H * W], bits16(torch.cat(hosts16, dim=1))) and not g16[:, wc.H * W:].any() and p16.written(), ctx
                assert np.array_equal(g32[:, :wc.H * W], np.hstack(wide).view(np.uint32)) and not g32[:, wc.H * W:].any() and p32.written(), ctx
            ran("sgl_hop_concat_bf16", W, layout)
            ran("sgl_hop_concat_bf16_f32", W, layout)
    # a row of n_hops * d + pad_cols columns beyond the limit is refused by name (d itself is inside it)
    top = wc.C["SGL_MAX_WIDTH"]
    d = top // 2 + 1
    for entry in ("sgl_hop_concat_bf16", "sgl_hop_concat_bf16_f32"):
        rc, msg = code(entry, 2, ptrs, (ctypes.c_int64 * 2)(d, d), P(o32.t), 2 * d, 0, 0, d)
        assert rc == _lib.SGL_ERR_UNSUPPORTED and msg == f"{entry}: n_hops * d + pad_cols={2 * d} is wider than SGL_MAX_WIDTH={top}", (rc, msg)
    family_report("bf16_agg")


# ---- row-wise aggregators beyond their register layouts ----------------------------------------------------------------------------------
def test_rowwise_beyond_the_register_layouts(cuda):
    """sgl_nafs_f32 / sgl_nafs_padded_f32 above 512 columns (the weight kernel, then the weighted sum; the padded form zeroes its
    declared pad columns like the fused kernel does) and sgl_hop_rowdot_f32 on 64 lanes per row: weights, outputs and scores
    against float64 through truth_report, the float32 reference being the oracle's numpy statement"""
    for n, W in wc.shapes(wc.ALL4):
        for layout in (("padded", "offset") if W == wc.W_CAP else ("padded",)):
            hosts = wc.hops_host(n, W, wc.H)
            xs = [inp(h, cuda, layout) for h in hosts]
            ptrs, lds = _lib.hop_arrays(xs)
            f64 = [torch.from_numpy(h).double() for h in hosts]
            w64 = tc.nafs_weight(f64).numpy()
            y64 = tc.combine_over_smooth_distance_vectorised(f64).numpy()
            w32, y32 = oracle.nafs_weights(hosts), oracle.agg_over_smooth_distance(hosts)
            o, w = Out(n, W, cuda, layout), Out(n, wc.H, cuda, "offset")
            call("sgl_nafs_f32", wc.H, ptrs, lds, P(o.t), ld(o.t), P(w.t), ld(w.t), n, W)
            truth("sgl_nafs_f32", "W", n, W, w.t.cpu().numpy(), w32, w64)
            truth("sgl_nafs_f32", "out", n, W, o.t.cpu().numpy(), y32, y64)
            assert o.written() and w.written(), (n, W, layout)
            ran("sgl_nafs_f32", W, layout)
            if layout == "padded":
                pad = 8 - W % 4 if W % 4 else 4
                o2, w2 = Out(n, W + pad, cuda), Out(n, wc.H, cuda, "offset")
                call("sgl_nafs_padded_f32", wc.H, ptrs, lds, P(o2.t), ld(o2.t), pad, P(w2.t), ld(w2.t), n, W)
                got = o2.t.cpu().numpy()
                assert torch.equal(w2.t, w.t) and np.array_equal(got[:, :W], o.t.cpu().numpy()), (n, W, "padded = plain")
                assert not got[:, W:].view(np.uint32).any() and o2.written(), (n, W, "pad columns are zeros")
                truth("sgl_nafs_padded_f32", "out", n, W, got[:, :W], y32, y64)
                ran("sgl_nafs_padded_f32", W, layout)
            v = vector(W, 7 * (W % 101) + 1, 0.3)
            vp = dev._padded_vec(torch.from_numpy(v), W, cuda)
            s = Out(n, wc.H, cuda, "offset")
            call("sgl_hop_rowdot_f32", wc.H, ptrs, lds, P(vp), P(s.t), ld(s.t), n, W)
            truth("sgl_hop_rowdot_f32", "scores", n, W, s.t.cpu().numpy(), np.stack([(x * v).sum(1, dtype=np.float32) for x in hosts], 1),
                  np.stack([x.astype(np.float64) @ v for x in hosts], 1), cond=np.stack([np.abs(x).astype(np.float64) @ np.abs(v) for x in hosts], 1))
            assert s.written(), (n, W, layout)
            ran("sgl_hop_rowdot_f32", W, layout)
    family_report("rowwise")


def test_documented_width_limits(cuda):
    """the entry points whose header documents a narrower limit: right at the limit, refused one past it with the documented code,
    nothing launched (the outputs still hold the sentinel).  512: sgl_nafs_prefix_f32 (SGL_ERR_INVALID), sgl_nafs_bf16_f32, sgl_hop_gate_f32
    / _padded_f32, sgl_hop_recursive_f32, sgl_hop_rowdot2_f32 (SGL_ERR_UNSUPPORTED); 1 024: sgl_hop_colsum_f32 and its scratch size;
    256 floats: sgl_probe_gather_f32"""
    n, Hn = 9, wc.H
    INVALID, UNSUPPORTED = 1001, _lib.SGL_ERR_UNSUPPORTED
    for d, ok in ((512, True), (513, False)):
        hosts = wc.hops_host(n, d, Hn, seed=4)
        xs = [inp(h, cuda) for h in hosts]
        ptrs, lds = _lib.hop_arrays(xs)
        pad = 0                                                               # (at d = 512 the 64 x 2 lane layout has no lane left for pad columns)
        v = vector(d, 7 * d + 1, 0.3)
        vp = dev._padded_vec(torch.from_numpy(v), d, cuda, tail=torch.tensor([BIAS]))

        def expect(entry, rc_msg, outs, want_rc, text):
            rc, msg = rc_msg
            if ok:
                assert rc == 0 and all(q.written(p) for q, p in outs), (entry, d, rc, msg)
            else:
                assert rc == want_rc and text in msg and entry.replace("_padded", "") in msg, (entry, d, rc, msg)
                assert all(bool((ints(q.parent) == sentinel_of(q.parent)).all()) for q, _ in outs), (entry, d, "something was launched")
            ran(entry, d)

        # NAFS prefix sweep
        outs = [Out(n, d + pad, cuda) for _ in range(2)]
        optrs, olds = _lib.hop_arrays([q.t for q in outs])
        expect("sgl_nafs_prefix_f32", code("sgl_nafs_prefix_f32", Hn, ptrs, lds, 0b101, optrs, olds, pad, 0, 1.0, n, d),
               [(q, pad) for q in outs], INVALID, "rows of up to 512 floats")
        if ok:
            for h, q in zip((0, 2), outs):
                assert oracle.parity_ok(q.t.cpu().numpy()[:, :d], oracle.agg_over_smooth_distance(hosts[:h + 1]), 2e-5, rowwise=False), h
        # bf16 NAFS: bit-equal to widening first
        h16 = [rne(h) for h in hosts]
        x16 = [inp(h, cuda) for h in h16]
        p16, l16 = _lib.hop_arrays(x16)
        o, w = Out(n, d + pad, cuda), Out(n, Hn, cuda, "offset")
        expect("sgl_nafs_bf16_f32", code("sgl_nafs_bf16_f32", Hn, p16, l16, P(o.t), ld(o.t), pad, P(w.t), ld(w.t), n, d), [(o, pad), (w, 0)],
               UNSUPPORTED, "rows of more than 512 columns")
        if ok:
            y32, w32 = dev.nafs_aggregate([inp(h.float(), cuda) for h in h16], return_weights=True)
            assert torch.equal(o.t[:, :d], y32) and torch.equal(w.t, w32)
        # gate, both forms
        y64, w64, g64 = gate_reference(hosts, v, torch.float64)
        y32, w32, g32 = gate_reference(hosts, v, torch.float32)
        for entry in ("sgl_hop_gate_f32", "sgl_hop_gate_padded_f32"):
            padded = "padded" in entry                                         # the padded form reads its bias from the device (NaN)
            o, w, g_ = Out(n, d, cuda), Out(n, Hn, cuda, "offset"), Out(n, Hn, cuda, "offset")
            args = (Hn, ptrs, lds, P(vp), NAN if padded else BIAS, P(o.t), ld(o.t)) + ((0,) if padded else ()) + (P(w.t), ld(w.t), P(g_.t), ld(g_.t), n, d)
            expect(entry, code(entry, *args), [(o, 0), (w, 0), (g_, 0)], UNSUPPORTED, "d <= 512")
            if ok:
                truth(entry, "out", n, d, o.t.cpu().numpy()[:, :d], y32, y64)
                truth(entry, "W", n, d, w.t.cpu().numpy(), w32, w64)
                truth(entry, "G", n, d, g_.t.cpu().numpy(), g32, g64)
        # recursive gate
        wt = vector(2 * d, 11 * d + 3, 0.5 / d ** 0.5)
        dp = dev.round_up(d, 4)
        rv = torch.zeros(2 * dp + 4, dtype=torch.float32)
        rv[:d], rv[dp:dp + d], rv[2 * dp] = torch.from_numpy(wt[:d]), torch.from_numpy(wt[d:]), BIAS
        rv = rv.to(cuda)
        o, w, a, c = Out(n, d + pad, cuda), Out(n, Hn, cuda, "offset"), Out(n, Hn, cuda, "offset"), Out(n, Hn, cuda, "offset")
        expect("sgl_hop_recursive_f32", code("sgl_hop_recursive_f32", Hn, ptrs, lds, P(rv), NAN, P(o.t), ld(o.t), pad, P(w.t), ld(w.t), P(a.t), ld(a.t),
                                             P(c.t), ld(c.t), n, d), [(o, pad), (w, 0), (a, 0), (c, 0)], UNSUPPORTED, "d <= 512")
        if ok:
            ref = {}
            for dt in (torch.float64, torch.float32):
                ff = [torch.from_numpy(x).to(dt) for x in hosts]
                wv = torch.from_numpy(wt).to(dt)
                y, wr = recursive_step_by_step(ff, wv, torch.tensor([BIAS], dtype=torch.float32).to(dt))
                ref[dt] = (y, wr, torch.stack([f @ wv[:d] for f in ff], 1), torch.stack([f @ wv[d:] for f in ff], 1))
            conds = [torch.stack([t64(np.abs(x)) @ t64(np.abs(part)) for x in hosts], 1) for part in (wt[:d], wt[d:])]
            r64, r32 = ref[torch.float64], ref[torch.float32]
            truth("sgl_hop_recursive_f32", "out", n, d, o.t.cpu().numpy()[:, :d], r32[0], r64[0])
            truth("sgl_hop_recursive_f32", "W", n, d, w.t.cpu().numpy(), r32[1], r64[1])
            truth("sgl_hop_recursive_f32", "A", n, d, a.t.cpu().numpy(), r32[2], r64[2], cond=conds[0])
            truth("sgl_hop_recursive_f32", "C", n, d, c.t.cpu().numpy(), r32[3], r64[3], cond=conds[1])
        # the jk / ori_ref scores
        u = np.ascontiguousarray(hash_matrix(Hn, d, seed=17 * d + Hn) * np.float32(0.3))
        ud = inp(u, cuda)
        p_, (a_, a_ok) = Out(n, Hn - 1, cuda, "offset"), out_vec(n, cuda)
        rcm = code("sgl_hop_rowdot2_f32", Hn, ptrs, lds, P(ud), ld(ud), 0b101, P(vp), 1, Hn, P(p_.t), ld(p_.t), P(a_), n, d)
        expect("sgl_hop_rowdot2_f32", rcm, [(p_, 0)], UNSUPPORTED, "0 < d <= 512")
        if ok:
            assert a_ok()
            for what, res, terms in (("P", p_.t, [[(hosts[h], v)] for h in range(1, Hn)]), ("A", a_[:, None], [[(hosts[j], u[j]) for j in (0, 2)]])):
                truth("sgl_hop_rowdot2_f32", what, n, d, res.cpu().numpy(), torch.stack([sum(t32(x) @ t32(y_) for x, y_ in cc) for cc in terms], 1),
                      torch.stack([sum(t64(x) @ t64(y_) for x, y_ in cc) for cc in terms], 1),
                      cond=torch.stack([sum(t64(x).abs() @ t64(y_).abs() for x, y_ in cc) for cc in terms], 1))
    # column sums: 1 024
    for d, ok in ((1024, True), (1025, False)):
        hosts = wc.hops_host(n, d, Hn, seed=4)
        xs = [inp(h, cuda) for h in hosts]
        ptrs, lds = _lib.hop_arrays(xs)
        wgt = np.ascontiguousarray(hash_matrix(n, Hn, seed=9 * d + Hn))
        wd = inp(wgt, cuda, "offset")
        size = int(_lib.lib().sgl_hop_colsum_scratch(Hn, n, d))
        assert (size > 0) == ok
        ran("sgl_hop_colsum_scratch", d)
        scratch = torch.empty(max(size, 4), dtype=torch.float32, device=cuda)
        o = Out(Hn, d, cuda)
        rc, msg = code("sgl_hop_colsum_f32", Hn, ptrs, lds, P(wd), ld(wd), 1, P(o.t), ld(o.t), P(scratch), n, d)
        if ok:
            assert rc == 0 and o.written(), msg
            want = torch.stack([t64(f).t() @ t64(wgt)[:, h] for h, f in enumerate(hosts)])
            mag = torch.stack([t64(f).abs().t() @ t64(wgt)[:, h].abs() for h, f in enumerate(hosts)]).clamp_min(1e-30)
            assert float(((o.t.cpu().double() - want).abs() / mag).max()) <= 2e-6          # the bar of test_hop_colsum_is_the_weight_gradient_of_the_row_dots
        else:
            assert rc == UNSUPPORTED and msg == "sgl_hop_colsum_f32: needs <= 16 hops, d <= 1024 and 16-byte aligned rows", (rc, msg)
            assert bool((ints(o.parent) == SENT).all())
        ran("sgl_hop_colsum_f32", d)
    # the gather probe: rows of at most 256 floats; it writes nothing, so "right" is "runs and leaves its sink alone"
    table = inp(hash_matrix(64, 260, seed=3), cuda)
    idx = torch.arange(64, dtype=torch.int32, device=cuda)
    sink, sink_ok = out_vec(1, cuda)
    for rf, ok in ((256, True), (260, False)):
        rc = _lib.probe_lib().sgl_probe_gather_f32(P(table), ld(table), P(idx), 64, rf, 8, P(sink), _lib.current_stream_ptr())
        msg = _lib.probe_lib().sgl_probe_last_error().decode()
        torch.cuda.synchronize()
        assert (rc == 0) if ok else (rc == INVALID and msg.startswith("sgl_probe_gather_f32:")), (rf, rc, msg)
        ran("sgl_probe_gather_f32", rf)
    family_report("limits")


# ---- rows ----------------------------------------------------------------------------------------------------------------------------
def test_gathers_scatter_signature_and_generator(cuda):
    """sgl_gather_rows_f32 / _padded_f32, sgl_gather_hops_padded_f32 (both gather_hops_grid settings), sgl_scatter_rows_f32, the two
    bfloat16 gathers: bit-equal to numpy indexing; sgl_col_signature_f32 (1 025 launches of 1 024 columns at the widest) against its
    definition; sgl_synth_features against its numpy mirror"""
    for n, W in wc.shapes(wc.ALL4 + (wc.W_BF16,)):
        idx_h = np.array(([0, n - 1, 0, -1, -n] + list(range(n)))[:max(n, 5)], dtype=np.int64)
        m = len(idx_h)
        idx = torch.from_numpy(idx_h).to(cuda)
        hosts = wc.hops_host(n, W, wc.H, seed=1)
        if W != wc.W_BF16:
            for layout in (("padded", "offset") if W == wc.W_CAP else ("padded",)):
                xs = [inp(h, cuda, layout) for h in hosts]
                o = Out(m, W, cuda, layout)
                call("sgl_gather_rows_f32", P(xs[0]), ld(xs[0]), n, P(idx), m, P(o.t), ld(o.t), W)
                assert np.array_equal(o.t.cpu().numpy(), hosts[0][idx_h]) and o.written(), (n, W, layout)
                ran("sgl_gather_rows_f32", W, layout)
                perm_h = np.random.default_rng(3).permutation(m).astype(np.int64)
                o = Out(m, W, cuda, layout)
                dev.scatter_rows(xs[2], torch.from_numpy(np.where(idx_h < 0, idx_h + n, idx_h)).to(cuda), torch.from_numpy(perm_h).to(cuda), o.t)
                want = np.empty((m, W), np.float32)
                want[perm_h] = hosts[2][idx_h]
                assert np.array_equal(o.t.cpu().numpy(), want) and o.written(), (n, W, layout)
                ran("sgl_scatter_rows_f32", W, layout)
            xs = [inp(h, cuda) for h in hosts]
            pad = dev.round_up(W, 4) - W + 4
            o, o2 = Out(m, W + pad, cuda), Out(m, W, cuda)
            call("sgl_gather_rows_padded_f32", P(xs[1]), ld(xs[1]), n, P(idx), m, P(o.t), ld(o.t), W, pad)
            dev.gather_rows(xs[1], idx, out=o2.t)
            got = o.t.cpu().numpy()
            assert np.array_equal(got[:, :W], hosts[1][idx_h]) and not got[:, W:].view(np.uint32).any() and o.written(), (n, W)
            assert np.array_equal(o2.t.cpu().numpy(), hosts[1][idx_h]), (n, W)          # (the wrapper declares the pad of the view it is given)
            ran("sgl_gather_rows_padded_f32", W)
            ptrs, lds = _lib.hop_arrays(xs)
            for grid in (1, 0):
                outs = [Out(m, W + pad, cuda) for _ in hosts]
                optrs, olds = _lib.hop_arrays([q.t for q in outs])
                with tuned(gather_hops_grid=grid):
                    call("sgl_gather_hops_padded_f32", wc.H, ptrs, lds, n, P(idx), m, optrs, olds, W, pad)
                for h, q in enumerate(outs):
                    got = q.t.cpu().numpy()
                    assert np.array_equal(got[:, :W], hosts[h][idx_h]) and not got[:, W:].view(np.uint32).any() and q.written(), (n, W, grid, h)
                ran("sgl_gather_hops_padded_f32", W, f"padded grid={grid}")
            # the column signature of the columns the kernel reads (up to 3 pad columns are signed with the rest)
            dw = dev.round_up(W, 4)
            sig = dev.column_signature(xs[0])
            assert sig is not None and sig.numel() == dw
            read = np.ascontiguousarray(torch.as_strided(xs[0], (n, dw), (xs[0].stride(0), 1), xs[0].storage_offset()).cpu().numpy())
            with np.errstate(over="ignore"):
                want = sig_mix(read.view(np.uint32), np.arange(n, dtype=np.uint64)[:, None]).sum(axis=0, dtype=np.uint64)
            assert np.array_equal(sig.cpu().numpy().view(np.uint64), want), (n, W)
            ran("sgl_col_signature_f32", W)
            # the generator: d data columns, zeros up to the pitch
            o = Out(n, W + pad, cuda)
            rows = torch.as_strided(o.parent, (n, ld(o.t)), (ld(o.t), 1))
            _lib.check_probe(_lib.probe_lib().sgl_synth_features(ctypes.c_uint64(9), 5, n, W, ld(o.t), P(rows), _lib.current_stream_ptr()), "sgl_synth_features")
            got = rows.cpu().numpy()
            assert np.array_equal(got[:, :W], synthetic.hashed_features_numpy(9, np.arange(5, 5 + n), W)) and not got[:, W:].view(np.uint32).any(), (n, W)
            assert bool((ints(o.parent)[n:] == SENT).all())
            ran("sgl_synth_features", W)
        if W in (wc.W_CAP, wc.W_ODD, wc.W_BF16):
            h16 = [rne(h) for h in hosts]
            for layout in (("padded", "offset") if W == wc.W_CAP else ("padded",)):
                x16 = [inp(h, cuda, layout) for h in h16]
                o, o2 = Out(m, W, cuda, layout), Out(m, W, cuda, layout)
                call("sgl_gather_rows_bf16_f32", P(x16[0]), ld(x16[0]), n, P(idx), m, P(o.t), ld(o.t), W, 0)
                dev.gather_rows(x16[0], idx, out=o2.t)
                want = h16[0].float().numpy()[idx_h]
                assert np.array_equal(o.t.cpu().numpy(), want) and np.array_equal(o2.t.cpu().numpy(), want) and o.written(), (n, W, layout)
                ran("sgl_gather_rows_bf16_f32", W, layout)
                outs = [Out(m, W, cuda, layout) for _ in h16]
                p16, l16 = _lib.hop_arrays(x16)
                optrs, olds = _lib.hop_arrays([q.t for q in outs])
                call("sgl_gather_hops_bf16_f32", wc.H, p16, l16, n, P(idx), m, optrs, olds, W, 0)
                assert all(np.array_equal(q.t.cpu().numpy(), h16[h].float().numpy()[idx_h]) and q.written() for h, q in enumerate(outs)), (n, W, layout)
                ran("sgl_gather_hops_bf16_f32", W, layout)
    family_report("rows")


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
EDGES = np.array([[0, 1], [1, 2], [2, 2], [-1, 0], [0, 1], [1, 0], [2, 1], [0, -2], [1, 1]], dtype=np.int64)      # a self pair, repeats, negatives


def test_edge_scores_and_edge_loss(cuda):
    """sgl_edge_dot_f32 (one- and two-matrix form) and sgl_edge_loss_grad_f32 (both loss modes; max_piece = 2, so node 1's row is cut
    and the fold runs) on a tiny edge list over rows of W columns scaled to unit length: scores, loss and dZ against float64 through
    truth_report with the sums of the absolute terms as cond, as their own tests compare them"""
    for n, W in wc.shapes(wc.ALL4):
        n = max(n, 3)
        a_h, b_h = (np.ascontiguousarray(wc.hops_host(n, W, 2, seed=6)[k] * np.float32(1.7 / np.sqrt(W))) for k in (0, 1))
        e = np.where(EDGES < 0, EDGES + n, EDGES)
        edges = torch.from_numpy(EDGES).to(cuda)
        for layout in (("padded", "offset") if W == wc.W_CAP else ("padded",)):
            ad, bd = inp(a_h, cuda, layout), inp(b_h, cuda, layout, 1e30)
            for two in (False, True):
                other_h, other = (b_h, bd) if two else (a_h, ad)
                o, o_ok = out_vec(len(EDGES), cuda)
                dev.edge_dot(ad, other, edges, out=o)
                x64, y64 = a_h[e[:, 0]].astype(np.float64), other_h[e[:, 1]].astype(np.float64)
                truth("sgl_edge_dot_f32", f"scores two={two}", n, W, o.cpu().numpy(), (a_h[e[:, 0]] * other_h[e[:, 1]]).sum(1, dtype=np.float32),
                      (x64 * y64).sum(1), cond=(np.abs(x64) * np.abs(y64)).sum(1))
                assert o_ok(), (n, W, layout, two)
            ran("sgl_edge_dot_f32", W, layout)
            labels = elc.labels_for(len(EDGES))
            plan = EdgePlan(EDGES, labels, n, max_piece=2, device=cuda)
            assert plan.n_partial > 0 and plan.fold.shape[0] > 0
            for mode in ("sigmoid", "none"):
                ref = elc.step_references(a_h, EDGES, labels, mode)
                dz = Out(n, W, cuda, layout)
                score, s_ok = out_vec(len(EDGES), cuda)
                dev.edge_loss_grad(ad, plan, mode, w=1.0 / len(EDGES), dz=dz.t, score=score)
                loss = float(plan.piece_loss.double().sum()) / len(EDGES)
                truth("sgl_edge_loss_grad_f32", f"dZ {mode}", n, W, dz.t.cpu().numpy(), ref["ref32"][1], ref["truth"][1], cond=ref["cond"][1])
                truth("sgl_edge_loss_grad_f32", f"loss {mode}", n, W, [loss], [ref["ref32"][0]], [ref["truth"][0]], cond=[ref["cond"][0]])
                o, _ = out_vec(len(EDGES), cuda)
                dev.edge_dot(ad, ad, edges, out=o)
                assert torch.equal(score, o) and s_ok() and dz.written(), (n, W, layout, mode)      # the logits are edge_dot's, bit for bit
            ran("sgl_edge_loss_grad_f32", W, layout)
    family_report("edges")


# ---- losses and k-means --------------------------------------------------------------------------------------------------------------
def test_class_loss_at_c_equal_W(cuda):
    """sgl_class_loss_grad_f32 with c = W classes (the streaming kernel; c is a loop bound and the arg-max index): loss, dZ against
    float64 through truth_report (the cond of class_loss_common), the predicted class against torch's CPU max on rows with exact
    ties, NaNs and one all-NaN row"""
    for n, W in wc.shapes(wc.ALL4):
        rows = max(n, 8)                                                       # the arg-max cases come in groups of 8 rows
        z, y = clc.inputs(W, n=rows)
        y = y.copy()
        y[0], y[rows - 1] = W - 1, 0                                           # the last and the first class are somebody's label
        if rows > 2:
            y[1] = clc.IGNORE
        for layout in (("padded", "offset") if W == wc.W_CAP else ("padded",)):
            zd, yd = inp(z, cuda, layout), torch.from_numpy(y).to(cuda)
            w = clc.weight(y, W)
            dz = Out(rows, W, cuda, layout)
            (rl, rl_ok), (pred, p_ok) = out_vec(rows, cuda), out_vec(rows, cuda, torch.int64)
            dev.class_loss_grad(zd, yd, w, dz=dz.t, row_loss=rl, pred=pred)
            ref = clc.step_references(z, y)
            r32 = clc.restated_step(z, y)
            truth("sgl_class_loss_grad_f32", "dZ", rows, W, dz.t.cpu().numpy(), r32[1], ref["truth"][1], cond=ref["cond"][1])
            truth("sgl_class_loss_grad_f32", "loss", rows, W, [float(rl.double().sum()) * w], [r32[0]], [ref["truth"][0]], cond=[ref["cond"][0]])
            uniq = clc.unique_maximum(z)
            assert np.array_equal(pred.cpu().numpy()[uniq], clc.reference_pred(z)[uniq]) and dz.written() and rl_ok() and p_ok(), (rows, W, layout)
            # ties, NaNs, a row of NaN alone: the first index wins, as output.max(1)[1] on the CPU
            za = clc.argmax_cases(W, n=8)
            za[7] = np.nan
            pred, p_ok = out_vec(8, cuda, torch.int64)
            dev.class_loss_grad(inp(za, cuda, layout), None, 1.0, pred=pred)
            assert np.array_equal(pred.cpu().numpy(), clc.reference_pred(za)) and p_ok() and int(pred[7]) == 0, (W, layout)
            # the NaN row poisons its own loss and gradient alone
            zn = z.copy()
            zn[rows - 1, W // 2] = np.nan
            dz = Out(rows, W, cuda, layout)
            rl, _ = out_vec(rows, cuda)
            dev.class_loss_grad(inp(zn, cuda, layout), yd, w, dz=dz.t, row_loss=rl)
            got = dz.t.cpu().numpy()
            assert np.isnan(got[rows - 1]).all() and np.isfinite(got[:rows - 1]).all() and bool(torch.isnan(rl[rows - 1])) and dz.written(), (W, layout)
            ran("sgl_class_loss_grad_f32", W, layout)


def test_centre_kernels_at_d_equal_W_and_k_equal_4100(cuda):
    """sgl_kmeans_assign_f32 and sgl_cluster_loss_grad_f32 with d = W (streaming kernels) and k in {1, 3}, and with the width as a
    COUNT: k = 4 100 centres of 7 columns, staged in three LDS tiles.  Distances, loss and dX against float64 through truth_report;
    labels are compared on the rows that kmeans_common's rule does not call near a tie"""
    cases = [(n, W, k) for n, W in wc.shapes(wc.ALL4) for k in wc.KS] + [(9, wc.D_NARROW, wc.K_WIDE)]
    for n, d, k in cases:
        x, c, y = cll.inputs(d, k, n=max(n, k) + 4)                            # (min(3, k) centres are exact copies of drawn rows: zero distances
                                                                               # occur, and with four spare rows no case has zero distances alone)
        x, y = x[:n], y[:n]
        rec_w = d if k != wc.K_WIDE else k                                     # the width the case is recorded under
        for layout in (("padded", "offset") if d in (wc.W_CAP, wc.D_NARROW) else ("padded",)):
            xd, cd, yd = inp(x, cuda, layout), inp(c, cuda, layout, 1e30), torch.from_numpy(y).to(cuda)
            (labels, l_ok), (mind, m_ok) = out_vec(n, cuda, torch.int64), out_vec(n, cuda)
            call("sgl_kmeans_assign_f32", P(xd), ld(xd), n, d, P(cd), ld(cd), k, P(labels), P(mind))
            l2, m2 = dev.kmeans_assign(xd, cd)
            dist64 = kc.distances64(x, c)
            want = dist64.argmin(1)
            d1 = dist64[np.arange(n), want]
            assert dist64.max() > 0                                            # not blind: some row is no copy of a centre
            near = (np.partition(dist64, 1, axis=1)[:, 1] - d1) <= kc.tau(d) * np.partition(dist64, 1, axis=1)[:, 1] if k > 1 else np.zeros(n, bool)
            ref32 = np.stack([((x - cj) ** 2).sum(1, dtype=np.float32) for cj in c], 1).min(1)
            truth("sgl_kmeans_assign_f32", f"mindist k={k}", n, d, mind.cpu().numpy(), ref32, d1)
            assert np.array_equal(labels.cpu().numpy()[~near], want[~near]) and l_ok() and m_ok(), (n, d, k, layout)
            if n > 1 and k > 1:
                assert torch.equal(labels, l2) and torch.equal(mind, m2), (n, d, k, layout)
            else:       # the wrapper passes a one-row matrix with pitch d (_lib.leading_dim): at an odd d that is another lane size, hence
                        # another summation order (documented: the order depends on d and the layout) -- the same bar, not the same bits
                truth("sgl_kmeans_assign_f32", f"mindist (wrapper) k={k}", n, d, m2.cpu().numpy(), ref32, d1)
                assert np.array_equal(l2.cpu().numpy()[~near], want[~near]), (n, d, k, layout)
            ran("sgl_kmeans_assign_f32", rec_w, f"{layout} k={k} d={d}")

            dx = Out(n, d, cuda, layout)
            rl, rl_ok = out_vec(n, cuda)
            dev.cluster_loss_grad(xd, cd, yd, 1.0 / n, dx=dx.t, row_loss=rl)
            ref = cll.step_references(x, c, y)
            r32 = cll.restated_step(x, c, y)
            truth("sgl_cluster_loss_grad_f32", f"dX k={k}", n, d, dx.t.cpu().numpy(), r32[1], ref["truth"][1], cond=ref["cond"][1])
            truth("sgl_cluster_loss_grad_f32", f"loss k={k}", n, d, [float(rl.double().sum()) / n], [r32[0]], [ref["truth"][0]], cond=[ref["cond"][0]])
            assert dx.written() and rl_ok(), (n, d, k, layout)
            ran("sgl_cluster_loss_grad_f32", rec_w, f"{layout} k={k} d={d}")
    family_report("losses")


# ---- the record against the table ---------------------------------------------------------------------------------------------------------
def test_zz_every_case_of_the_table_ran():
    """(last in the file) every entry point of wide_common.CASES ran at every width its row names; run the whole file for this one"""
    missing = {e: sorted(set(c.widths) - {w for w, _ in RAN[e]}) for e, c in wc.CASES.items() if set(c.widths) - {w for w, _ in RAN[e]}}
    # the centre kernels record their k = 4 100 case under K_WIDE, the concat its 2^31 case under d = 33 554 433 (tiered by memory)
    assert not missing, missing
    assert all(any(w == wc.K_WIDE and "k=4100" in lay for w, lay in RAN[e]) for e in ("sgl_kmeans_assign_f32", "sgl_cluster_loss_grad_f32"))
    total = sum(len(v) for v in RAN.values())
    print(f"\n[wide rows] {total} (entry point, width, layout) cases over {len(RAN)} entry points; "
          f"2^31 concat ran: {any(w == wc.HUGE['d'] for w, _ in RAN['sgl_hop_concat_f32'])}")

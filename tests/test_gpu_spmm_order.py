"""Default ("fast") order SpMM, bit for bit, in every compiled kernel variant, on a real MI355X: run with `-m gpu`.

The default order of spmm_kernel (csrc/sgl_spmm.hip, run_rows: "slot of a non-zero = its index WITHIN ITS ROW mod R") and of
spmm_bf16_kernel (csrc/sgl_spmm_bf16.hip, header "Numerics" and run_rows) is deterministic, so it is restated on the CPU
(oracle.oracle_spmm_slots, oracle/spmm_ref.c) and compared exactly: fp32 results as 32-bit patterns, bf16 results as 16-bit
patterns, NaNs by position.  There is NO tolerance anywhere in this file.

Which template instance runs is decided by spmm_impl / spmm_slice (the lane width) and sgl::spmm_layout (csrc/sgl_core.cpp: the
lane layout) from widths, pitches, pointer alignment, the average row length and the tuning keys.  That rule is restated in spmm_order_common.dispatch, and every launch made here is checked against
the name of the kernel that really ran, as the profiler reports it.  The model's R is 64 / GROUP of that kernel."""
import contextlib

import numpy as np
import pytest
import torch

import oracle
from inputs import hash_matrix
from sgl_amd import _lib
from sgl_amd import device as dev
from spmm_order_common import (TUNING_DEFAULTS, TUNING_KEYS, TUNING_VALUES, compiled_variants, cut_rule, default_long_row_nnz,
                               dense_graph, dispatch, medium_graph, parse_kernel_name)
from test_gpu_bf16 import bits, long_row_graph, rne

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
# widths per lane width W (elements per lane access), contiguous: lanes = d / W of 5 (<= 8), 13 (<= 16), 25 (<= 32), 63 / 64
# (<= 64), 125 (two chunks), 255 (four chunks), then two and three column slices (one launch covers 256 * W columns)
WIDTHS = {
    "bf16": {8: [40, 104, 200, 512, 1000, 2040, 2056, 4104], 4: [20, 52, 100, 252, 500, 1020, 1028, 2052],
             2: [10, 26, 50, 126, 250, 510, 514, 1026], 1: [5, 13, 25, 63, 125, 255, 257, 513]},
    "f32": {4: [20, 52, 100, 252, 500, 1020, 1028, 2052], 2: [10, 26, 50, 126, 250, 510, 514, 1026],
            1: [5, 13, 25, 63, 125, 255, 257, 513]},
}


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


# ---- graphs, handles, inputs, the model ------------------------------------------------------------------------------------
_GRAPHS = {}


def graph(name):
    """(n, rowptr, col, val) of "sparse" (the long-row graph of test_gpu_bf16.py, < 12 nnz per row), "medium" (12 .. 40) or
    "dense" (>= 40): canonical CSR, some empty rows, three rows of >= 900 non-zeros"""
    if name not in _GRAPHS:
        a = {"sparse": long_row_graph, "medium": medium_graph, "dense": dense_graph}[name]()
        deg = np.diff(a.indptr)
        avg = a.nnz / a.shape[0]
        assert a.has_canonical_format and (deg == 0).sum() > 0 and (deg >= 900).sum() == 3
        assert {"sparse": avg < 12, "medium": 12 <= avg < 40, "dense": avg >= 40}[name], avg
        _GRAPHS[name] = (a.shape[0], a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float32))
    return _GRAPHS[name]


def to_dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def handles(name, cuda, strict=False):
    """{label: (DeviceCSR, the long_row_nnz the model needs)}: explicit long_row_nnz = 128, the default threshold, 64-nnz items,
    and a random row permutation behind a row map.  The number of pieces is asserted against the cut rule."""
    n, ptr, col, val = graph(name)
    if strict:
        csr = dev.DeviceCSR(to_dev(ptr, cuda), to_dev(col, cuda), to_dev(val, cuda), (n, n), strict=True)
        assert csr.info()["n_pieces"] == 0
        return {"strict": (csr, -1)}
    out = {}
    for label, kw in (("lr128", dict(long_row_nnz=128)), ("default", dict()), ("item64", dict(long_row_nnz=128, item_nnz=64))):
        out[label] = (dev.DeviceCSR(to_dev(ptr, cuda), to_dev(col, cuda), to_dev(val, cuda), (n, n), **kw),
                      kw.get("long_row_nnz") or default_long_row_nnz(len(col)))
    perm = np.random.default_rng(7).permutation(n)
    deg = np.diff(ptr)
    p_ptr = np.concatenate([[0], np.cumsum(deg[perm])]).astype(np.int64)
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in perm])
    mapped = dev.DeviceCSR(to_dev(p_ptr, cuda), to_dev(col[take], cuda), to_dev(val[take], cuda), (n, n), long_row_nnz=128)
    out["rowmap"] = (mapped.set_rowmap(to_dev(perm.astype(np.int32), cuda)), 128)
    for label, (csr, lr) in out.items():
        want = len(cut_rule(ptr, lr))
        assert want >= 3 and csr.info()["n_pieces"] == want and csr.info()["n_long_rows"] == int((deg > lr).sum()), (label, csr.info())
    return out


_X = {}


def x_host(name, dtype, d, seed=0):
    """the dense operand as float32 on the host; for bf16 the stored values, widened (exact)"""
    key = (name, dtype, d, seed)
    if key not in _X:
        x = hash_matrix(graph(name)[0], d, seed=d + seed)
        _X[key] = rne(x).float().numpy() if dtype == "bf16" else x
        if len(_X) > 24:
            _X.pop(next(iter(_X)))
    return _X[key]


def result_bits(y, dtype):
    """the bit patterns a kernel must store for the fp32 sums y: the floats themselves, or their one rounding to bf16"""
    return bits(rne(y)) if dtype == "bf16" else np.ascontiguousarray(y, dtype=np.float32).view(np.uint32)


def device_bits(t):
    return bits(t) if t.dtype == torch.bfloat16 else t.detach().cpu().contiguous().numpy().view(np.uint32)


def same_bits(got, want):
    """equal bit patterns; NaNs compare by position"""
    if got.dtype == np.uint16:
        gn, wn = (got & 0x7fff) > 0x7f80, (want & 0x7fff) > 0x7f80
    else:
        gn, wn = (got & 0x7fffffff) > 0x7f800000, (want & 0x7fffffff) > 0x7f800000
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(got[~gn], want[~wn])


def n_diff(got, want):
    return int((got != want).sum())


def model_sums(mat, x, slices, lr, strict):
    """fp32 sums of the product in the order of the kernels that ran: per column slice, R = 64 / GROUP"""
    n, ptr, col, val = mat
    if strict:
        return oracle.oracle_spmm(ptr, col, val, x)
    y = np.empty((n, x.shape[1]), np.float32)
    for c0, dc, var in slices:
        y[:, c0:c0 + dc] = oracle.oracle_spmm_slots(ptr, col, val, x[:, c0:c0 + dc], 64 // var[1], lr)
    return y


_MODEL = {}


def model_bits(name, dtype, d, slices, lr, strict, seed=0):
    """evaluated once per (graph, width, operand, R per slice, long_row_nnz) and re-used by every variant that shares those"""
    key = (name, dtype, d, seed, -1 if strict else lr, strict, tuple((c0, dc, 1 if strict else 64 // v[1]) for c0, dc, v in slices))
    if key not in _MODEL:
        _MODEL[key] = result_bits(model_sums(graph(name), x_host(name, dtype, d, seed), slices, lr, strict), dtype)
        if len(_MODEL) > 32:
            _MODEL.pop(next(iter(_MODEL)))
    return _MODEL[key]


def make_mat(kind, n, d, dtype, cuda, fill=None):
    """[n, d] device matrix: "contig", "padded" (alloc_rows: the library's row pitch), or ("off", k): columns k .. k + d of a
    wider aligned matrix, so that the pointer is only aligned to k elements"""
    tdt = TORCH_DTYPE[dtype]
    if kind == "contig":
        t = torch.empty((n, d), dtype=tdt, device=cuda)
    elif kind == "padded":
        t = dev.alloc_rows(n, d, cuda, dtype=tdt)
    else:
        wide = torch.zeros((n, dev.round_up(d + 8, 8)), dtype=tdt, device=cuda)
        assert wide.data_ptr() % 16 == 0
        t = wide[:, kind[1]:kind[1] + d]
    if fill is not None:
        t.copy_(torch.from_numpy(fill).to(tdt))
    return t


def ld_of(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def expected_dispatch(dtype, name, x, y, strict, tuning=None, acc=None):
    n, ptr, col, _ = graph(name)
    return dispatch(dtype, x.shape[1], ld_of(x), ld_of(y), x.data_ptr(), y.data_ptr(), strict, len(col) / n, tuning,
                    None if acc is None else (ld_of(acc), acc.data_ptr()))


@contextlib.contextmanager
def tuned(**kw):
    saved = {k: _lib.get_tuning(k) for k in TUNING_KEYS}
    try:
        for k in TUNING_KEYS:
            _lib.set_tuning(k, kw.get(k, TUNING_DEFAULTS[k]))
        yield
    finally:
        for k, v in saved.items():
            _lib.set_tuning(k, v)


class Trace:
    """Runs launches under torch.profiler and checks, at exit, that the spmm_kernel / spmm_bf16_kernel instances that really
    ran are, in order, the ones `expect()` announced (the fix-up kernels and everything else are ignored)."""

    def __init__(self, dtype):
        self.kind, self.expected, self.seen = dtype, [], set()

    def expect(self, label, slices):
        self.expected += [(label, v) for _, _, v in slices]

    def __enter__(self):
        from torch.profiler import ProfilerActivity, profile
        self.prof = profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA])
        self.prof.__enter__()
        return self

    def __exit__(self, et, ev, tb):
        torch.cuda.synchronize()
        self.prof.__exit__(et, ev, tb)
        if et is not None:
            return False
        from torch.autograd import DeviceType
        evs = sorted((e for e in self.prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
        got = [p for p in (parse_kernel_name(e.name) for e in evs) if p is not None]
        assert len(got) == len(self.expected), (len(got), len(self.expected), got[:3], self.expected[:3])
        wrong = [(i, lab, g, w) for i, (g, (lab, w)) in enumerate(zip(got, self.expected)) if g != (self.kind, w)]
        assert not wrong, (len(wrong), wrong[:8])
        self.seen = {g[1] for g in got}
        return False


def run_spmm(tr, bad, label, dtype, name, csr, lr, strict, d, xd, ykind, cuda, tuning=None, seed=0):
    """one product into a fresh Y pre-filled with a sentinel: announce the kernels, compare the bits with the model"""
    n = graph(name)[0]
    y = make_mat(ykind, n, d, dtype, cuda)
    y.fill_(7.0)
    slices = expected_dispatch(dtype, name, xd, y, strict, tuning)
    tr.expect(label, slices)
    csr.spmm(xd, out=y)
    got, want = device_bits(y), model_bits(name, dtype, d, slices, lr, strict, seed)
    if not same_bits(got, want):
        bad.append((label, n_diff(got, want)))
    return slices


# ---- the production rule, untuned, on all three graphs -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_default_rule_every_width_bit_exact(cuda, dtype):
    """No tuning key set: the kernel the library itself picks for each graph (U from the average row length) and width, under four
    plans of the same matrix; all four give the model's bits.  Asserts the U levels of production are really reached."""
    bad, seen_by_graph = [], {}
    with tuned():
        for name in ("sparse", "medium", "dense"):
            n = graph(name)[0]
            hs = handles(name, cuda)
            with Trace(dtype) as tr:
                for w, widths in WIDTHS[dtype].items():
                    for d in widths:
                        xd = make_mat("contig", n, d, dtype, cuda, x_host(name, dtype, d))
                        for label, (csr, lr) in hs.items():
                            sl = run_spmm(tr, bad, (name, d, label), dtype, name, csr, lr, False, d, xd, "contig", cuda)
                            assert all(v[0] == w for _, _, v in sl), (d, sl)
                        assert len(sl) == {0: 1, 1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 2, 7: 3}[widths.index(d)], (d, sl)
            seen_by_graph[name] = tr.seen
    assert not bad, (len(bad), bad[:10])
    wmax = 8 if dtype == "bf16" else 4
    tail = (0,) if dtype == "f32" else ()
    # one row per step: 4 / 8 / 16 gathers in flight below 12 / below 40 / from 40 non-zeros per row
    for name, u in (("sparse", 4), ("medium", 8), ("dense", 16)):
        assert (wmax, 64, 1, u) + tail in seen_by_graph[name], (name, sorted(seen_by_graph[name]))
    # packed layouts: 8 per slot; bf16 takes 16 from 40 non-zeros per row on (the products-shaped d = 100 hop)
    for name in ("sparse", "medium", "dense"):
        u = 16 if (dtype == "bf16" and name == "dense") else 8
        assert {(wmax, 8, 1, u) + tail, (wmax, 16, 1, u) + tail} <= seen_by_graph[name], (name, sorted(seen_by_graph[name]))
        assert {(wmax, 64, 2, 4) + tail, (wmax, 64, 4, 2) + tail, (1, 64, 4, 2) + tail} <= seen_by_graph[name]
    print(f"{dtype} default rule: {len(set().union(*seen_by_graph.values()))} distinct kernel variants without any tuning key")


LAYOUT_PAIRS = [("contig", "contig"), ("padded", "padded"), ("contig", "padded"), ("padded", "contig"),
                (("off", 1), ("off", 1)), (("off", 2), ("off", 2)), (("off", 4), ("off", 4)),
                (("off", 1), "padded"), ("padded", ("off", 2)), (("off", 4), "contig")]


@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts_and_alignment_fallback_bit_exact(cuda, dtype):
    """contiguous, row-padded and mixed X / Y pitches, and X / Y as column-offset views of a wider matrix: there the pointer
    alignment, not d, forces the narrower lane width, which must show in the kernel name"""
    bad = []
    with tuned():
        for name in ("sparse", "dense"):
            n = graph(name)[0]
            hs = handles(name, cuda)
            with Trace(dtype) as tr:
                for d in (16, 100, 104, 264):
                    for xk, yk in LAYOUT_PAIRS:
                        xd = make_mat(xk, n, d, dtype, cuda, x_host(name, dtype, d))
                        for label, (csr, lr) in hs.items():
                            sl = run_spmm(tr, bad, (name, d, xk, yk, label), dtype, name, csr, lr, False, d, xd, yk, cuda)
                        w = sl[0][2][0]
                        if d % 8 == 0 and xk == yk and xk[0] == "off":       # d itself would allow the widest lanes
                            assert w == (min(xk[1], 8) if dtype == "bf16" else min(xk[1], 4)), (d, xk, sl)
                        if d % 8 == 0 and xk == yk == "padded":
                            assert w == (8 if dtype == "bf16" else 4)
                        if d == 100 and dtype == "bf16" and "contig" in (xk, yk):
                            assert w <= 4                                     # a 100-element pitch is not a multiple of 8
    assert not bad, (len(bad), bad[:10])


# ---- every compiled variant ---------------------------------------------------------------------------------------------------
def tuned_cases(dtype):
    """(d, tuning): with 5 lanes every GROUP can be forced and every level of launch_u chosen; 125 and 255 lanes give the two-
    and four-chunk layouts; then the lane-width cap, wavefronts per block, block order"""
    f32 = dtype == "f32"
    cases = []
    for w in WIDTHS[dtype]:
        for nt in ((0, 1) if f32 else (0,)):
            for group in (0, 16, 32, 64):
                for un in ((1, 3, 2, 4) if f32 else (1, 3, 2)):
                    cases.append((5 * w, dict(spmm_group=group, spmm_unroll=un, spmm_nt=nt)))
            for d in (125 * w, 255 * w):
                for un in (1, 3):
                    cases.append((d, dict(spmm_unroll=un, spmm_nt=nt)))
    wmax = max(WIDTHS[dtype])
    for d in (13 * wmax, 64 * wmax + 2 * wmax):
        for vec in (1, 2):
            cases.append((d, dict(spmm_vec=vec)))
    for d in (5 * wmax, 100):
        for waves in (1, 2, 4):
            for remap in (0, 1):
                cases.append((d, dict(spmm_waves=waves, spmm_xcd_remap=remap)))
    return cases


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_compiled_variant_bit_exact(cuda, dtype):
    """The tuning keys reach every template instance of the launch tables (spmm_order_common.compiled_variants restates them:
    sgl_spmm_bf16.hip launch_u / launch_group / the bv switch; sgl_spmm.hip launch_nt / launch_u / launch_group / the vec
    switch).  Each is run under four plans on the dense graph (most rows cross a 64-element slice of the (col, val) stream) and
    once on the sparse one, and gives the model's bits.  The set of instances seen must be the whole compiled set: an instance
    added later without a case here fails this test."""
    bad, seen = [], set()
    for name in ("dense", "sparse"):
        n = graph(name)[0]
        hs = handles(name, cuda)
        if name == "sparse":
            hs = {"default": hs["default"]}
        with Trace(dtype) as tr:
            for d, tuning in tuned_cases(dtype):
                with tuned(**tuning):
                    xd = make_mat("contig", n, d, dtype, cuda, x_host(name, dtype, d))
                    for label, (csr, lr) in hs.items():
                        run_spmm(tr, bad, (name, d, tuple(sorted(tuning.items())), label), dtype, name, csr, lr, False, d, xd, "contig",
                                 cuda, tuning)
        seen |= tr.seen
    compiled = compiled_variants(dtype)
    print(f"{dtype}: {len(seen)} distinct kernel variants seen, {len(compiled)} compiled")
    assert len(compiled) == (64 if dtype == "bf16" else 102)
    assert seen == compiled, (sorted(compiled - seen), sorted(seen - compiled))
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("dtype", DTYPES)
def test_strict_handles_ignore_every_tuning_key(cuda, dtype):
    """a strict-order handle is bit-equal to the reference chain (oracle_spmm) under every value of every tuning key: none of
    them may move it off one sequential chain per row (GROUP = 64 in the kernel name, spmm_group included)"""
    bad = []
    for name in ("dense", "sparse"):
        n = graph(name)[0]
        (csr, lr), = handles(name, cuda, strict=True).values()
        with Trace(dtype) as tr:
            for key in TUNING_KEYS:
                for value in TUNING_VALUES[key]:
                    with tuned(**{key: value}):
                        for d in (8, 16, 100, 257):
                            xd = make_mat("contig", n, d, dtype, cuda, x_host(name, dtype, d))
                            sl = run_spmm(tr, bad, (name, key, value, d), dtype, name, csr, lr, True, d, xd, "contig", cuda, {key: value})
                            assert all(v[1] == 64 for _, _, v in sl)
    assert not bad, (len(bad), bad[:10])


# ---- chains --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_of_three_hops_bit_exact(cuda, dtype):
    """spmm_chain over three hops; the model is fed ITS OWN previous hop (for bf16: rounded once per hop), never the device's"""
    bad, memo = [], {}
    with tuned():
        for name in ("sparse", "dense"):
            mat = graph(name)
            n = mat[0]
            for label, (csr, lr) in handles(name, cuda).items():
                with Trace(dtype) as tr:
                    for d in (16, 100, 257, 1028):
                        for kind in ("contig", "padded"):
                            cur = x_host(name, dtype, d)
                            x0 = make_mat(kind, n, d, dtype, cuda, cur)
                            outs = [make_mat(kind, n, d, dtype, cuda) for _ in range(3)]
                            prev = x0
                            plan = []
                            for k in range(3):
                                plan.append(expected_dispatch(dtype, name, prev, outs[k], False))
                                tr.expect((name, label, d, kind, k), plan[-1])
                                prev = outs[k]
                            key = (name, d, lr, tuple(tuple((c0, dc, v[1]) for c0, dc, v in sl) for sl in plan))
                            if key not in memo:
                                want = []
                                for sl in plan:
                                    y = model_sums(mat, cur, sl, lr, False)
                                    want.append(result_bits(y, dtype))
                                    cur = rne(y).float().numpy() if dtype == "bf16" else y
                                memo[key] = want
                            want = memo[key]
                            csr.spmm_chain(x0, 3, outs=outs)
                            for k in range(3):
                                got = device_bits(outs[k])
                                if not same_bits(got, want[k]):
                                    bad.append((name, label, d, kind, k, n_diff(got, want[k])))
    assert not bad, (len(bad), bad[:10])


# ---- the fused running aggregate ---------------------------------------------------------------------------------------------
ACC_CASES = [("sum", dict(mode="sum")), ("wsum", dict(mode="wsum", w=0.37)), ("mean", dict(mode="sum", divisor=3.0)),
             ("max", dict(mode="max")), ("min", dict(mode="min"))]


def acc_expected(kind, acc0, y):
    """the elementwise fp32 expression of acc_apply (both files), in numpy / torch on the CPU"""
    f = np.float32
    if kind == "sum":
        return acc0 + y
    if kind == "wsum":
        return acc0 + f(0.37) * y                       # rounded product, then add
    if kind == "mean":
        return (acc0 + y) / f(3.0)
    fn = torch.maximum if kind == "max" else torch.minimum      # torch's NaN rule: a NaN on either side wins
    return fn(torch.from_numpy(acc0), torch.from_numpy(np.ascontiguousarray(y))).numpy()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_aggregate_bit_exact(cuda, dtype):
    """spmm_acc on graphs with split rows (the fix-up kernel's aggregate branch, with a row map: through d_long_out), every mode,
    a width in column slices (the accumulator advances by c0 per slice), and accumulators that are padded, of odd pitch, and views
    offset by one and two floats: the lane width must drop as spmm_impl says (visible in the kernel name), Y must equal the
    unfused product of the same kernel and the model, ACC the fp32 expression over the STORED Y, nothing else may be written."""
    bad = []
    wide_d = 2056 if dtype == "bf16" else 1028
    for name in ("dense", "sparse"):
        mat = graph(name)
        n = mat[0]
        hs = handles(name, cuda)
        for label in ("lr128", "rowmap"):
            csr, lr = hs[label]
            with Trace(dtype) as tr:
                for d in (16, 104, wide_d):
                    xh = x_host(name, dtype, d)
                    xd = make_mat("padded", n, d, dtype, cuda, xh)
                    acc0 = hash_matrix(n, d, seed=77)
                    for akind in ("padded", "odd", 1, 2):
                        for kind, kw in ACC_CASES:
                            if akind == "padded":
                                base = dev.padded_parent(dev.alloc_rows(n, d, cuda))
                                off = 0
                            elif akind == "odd":
                                base = torch.empty((n, d + 1), device=cuda)
                                off = 0
                            else:
                                base = torch.empty((n, dev.round_up(d + 4, 4)), device=cuda)
                                off = akind
                            base.fill_(-3.0)
                            acc = base[:, off:off + d]
                            acc.copy_(torch.from_numpy(acc0))
                            y = make_mat("padded", n, d, dtype, cuda)
                            y.fill_(7.0)
                            plain = expected_dispatch(dtype, name, xd, y, False)
                            sl = expected_dispatch(dtype, name, xd, y, False, acc=(acc))
                            w0, w1 = plain[0][2][0], sl[0][2][0]
                            assert w1 == {"padded": w0, "odd": 1, 1: 1, 2: 2}[akind], (akind, w0, w1)
                            if d == wide_d:
                                assert len(sl) >= 2 and (akind == "padded" or len(sl) > len(plain))
                            tag = (name, label, d, akind, kind)
                            tr.expect(tag, sl)
                            with tuned():
                                csr.spmm_acc(xd, y, acc, **kw)
                            # the unfused product by the same kernel (lane width capped to the fused call's)
                            cap = {} if w1 == w0 else {"spmm_vec": w1}
                            y2 = make_mat("padded", n, d, dtype, cuda)
                            with tuned(**cap):
                                sl2 = expected_dispatch(dtype, name, xd, y2, False, cap)
                                assert [s[2] for s in sl2] == [s[2] for s in sl]
                                tr.expect(tag + ("unfused",), sl2)
                                csr.spmm(xd, out=y2)
                            got = device_bits(y)
                            if not same_bits(got, device_bits(y2)):
                                bad.append(tag + ("Y != unfused", n_diff(got, device_bits(y2))))
                            want = model_bits(name, dtype, d, sl, lr, False)
                            if not same_bits(got, want):
                                bad.append(tag + ("Y != model", n_diff(got, want)))
                            stored = y.detach().cpu().float().numpy()
                            a_want = np.ascontiguousarray(acc_expected(kind, acc0, stored), dtype=np.float32).view(np.uint32)
                            whole = base.cpu().numpy()
                            a_got = np.ascontiguousarray(whole[:, off:off + d]).view(np.uint32)
                            if not same_bits(a_got, a_want):
                                bad.append(tag + ("ACC", n_diff(a_got, a_want)))
                            rest = np.delete(whole, np.s_[off:off + d], axis=1)
                            if not (rest == -3.0).all():
                                bad.append(tag + ("wrote outside the accumulator",))
    assert not bad, (len(bad), bad[:10])


# ---- bf16: special values ------------------------------------------------------------------------------------------------------
def bf16_from_bits(b):
    return torch.from_numpy(np.asarray(b, np.uint16).view(np.int16)).view(torch.bfloat16)


def special_matrix(pad):
    """Hand-built rows over a 12-row operand whose row j holds one special value in every column.  pad > 0: every row gets `pad`
    terms on the all-zero operand row in front and behind, so that with long_row_nnz = 4 the same terms go through split rows."""
    BIG = 0x7f7f                                  # largest finite bf16, (2 - 2^-7) * 2^127
    xbits = [0x0000, 0x3f80, 0x7fc0, 0x7f80, 0xff80, BIG, 0x0001, 0x0003, 0x8000, 0x0d80, 0xff7f, 0x4000]
    #        zero    1.0     NaN     +inf    -inf    BIG  2^-133  3*2^-133 -0.0   2^-100  -BIG    2.0
    f = np.float32
    rows = [
        ([(1, 1.0)], None),                                          # 0: 1.0
        ([(2, 1.0), (1, 1.0)], "nan"),                               # 1: NaN stays NaN
        ([(3, 0.5), (1, 1.0)], 0x7f80),                              # 2: +inf stays +inf
        ([(4, 0.5), (1, 1.0)], 0xff80),                              # 3: -inf stays -inf
        ([(3, 1.0), (4, 1.0)], "nan"),                               # 4: inf - inf
        ([(5, f(1 + 2.0 ** -8))], 0x7f80),                           # 5: finite fp32 sum above the largest bf16 -> +inf
        ([(10, f(1 + 2.0 ** -8))], 0xff80),                          # 6: ... -> -inf
        ([(5, 1.0), (1, f(2.0 ** 118))], BIG),                       # 7: BIG + less than half an ulp of BIG stays BIG
        ([(5, 1.0), (5, 1.0)], 0x7f80),                              # 8: the fp32 sum itself overflows
        ([(1, f(1 + 2.0 ** -8))], 0x3f80),                           # 9: exact tie -> even (down)
        ([(1, f(1 + 3 * 2.0 ** -8))], 0x3f82),                       # 10: exact tie -> even (up)
        ([(1, f(1 + 2.0 ** -8)), (1, f(2.0 ** -23))], 0x3f81),       # 11: just above the tie -> up
        ([(6, 1.0)], 0x0001),                                        # 12: a bf16 subnormal input is kept
        ([(7, 0.5)], 0x0002),                                        # 13: fp32-subnormal sum 1.5 * 2^-133: tie -> even
        ([(6, 0.5)], 0x0000),                                        # 14: 0.5 * 2^-133: tie -> even (zero)
        ([(6, 0.75)], 0x0001),                                       # 15: 0.75 * 2^-133 -> the smallest subnormal
        ([(8, 1.0)], None),                                          # 16: 1 * -0.0 (+0.f + -0.f = +0.f)
        ([(9, f(-2.0 ** -100))], None),                              # 17: the product underflows to -0.f in the fmaf
        ([(11, -0.5), (1, 1.0)], 0x0000),                            # 18: exact cancellation -> +0
        ([], 0x0000),                                                # 19: empty row
    ]
    ptr, col, val = [0], [], []
    for terms, _ in rows:
        terms = [(0, 1.0)] * pad + terms + [(0, 1.0)] * pad if terms else terms
        col += [c for c, _ in terms]
        val += [v for _, v in terms]
        ptr.append(len(col))
    # square: the remaining rows are empty
    n = len(xbits) + len(rows)
    ptr += [ptr[-1]] * (n - len(rows))
    xb = xbits + [0x3f80] * (n - len(xbits))
    return n, np.asarray(ptr, np.int64), np.asarray(col, np.int32), np.asarray(val, np.float32), xb, [w for _, w in rows]


@pytest.mark.parametrize("pad", [0, 5])
def test_bf16_special_values(cuda, pad):
    """The contract of sgl_spmm_bf16.hip's header: NaN stays NaN, +-inf stays +-inf, overflow rounds to inf, subnormals are kept,
    ties go to even.  Hand-built rows with the expected 16-bit pattern written down, checked on the model first (torch-CPU rne
    of the fp32 model) and then on the device, whole rows and (pad = 5, long_row_nnz = 4) through split rows."""
    n, ptr, col, val, xb, want_rows = special_matrix(pad)
    lr = 4 if pad else 128
    # the non-canonical CSR (repeated columns) is deliberate: terms are terms
    csrs = {"fast": (dev.DeviceCSR(to_dev(ptr, cuda), to_dev(col, cuda), to_dev(val, cuda), (n, n), long_row_nnz=lr), lr, False),
            "strict": (dev.DeviceCSR(to_dev(ptr, cuda), to_dev(col, cuda), to_dev(val, cuda), (n, n), strict=True), -1, True)}
    assert csrs["fast"][0].info()["n_pieces"] == (3 * sum(1 for w in np.diff(ptr) if w > 4) if pad else 0)
    assert not pad or csrs["fast"][0].info()["n_pieces"] > 0
    bad = []
    with tuned(), Trace("bf16") as tr:
        for d in (1, 8, 16, 100, 264):
            xh = bf16_from_bits(np.repeat(np.asarray(xb, np.uint16)[:, None], d, axis=1))
            x = xh.float().numpy()
            for kind in ("contig", "padded"):
                xd = make_mat(kind, n, d, "bf16", cuda)
                xd.copy_(xh)
                assert np.array_equal(bits(xd), bits(xh))
                for label, (csr, lrn, strict) in csrs.items():
                    y = make_mat(kind, n, d, "bf16", cuda)
                    y.fill_(7.0)
                    sl = dispatch("bf16", d, ld_of(xd), ld_of(y), xd.data_ptr(), y.data_ptr(), strict, len(col) / n)
                    want = result_bits(model_sums((n, ptr, col, val), x, sl, lrn, strict), "bf16")
                    for r, w in enumerate(want_rows):                      # the model against the written-down contract
                        if w == "nan":
                            assert ((want[r] & 0x7fff) > 0x7f80).all(), (r, hex(want[r, 0]))
                        elif w is not None:
                            assert (want[r] == w).all(), (r, hex(want[r, 0]), hex(w))
                    assert (want[[0, 16]] == [[0x3f80], [0x0000]]).all() and ((want[17] & 0x7fff) == 0).all()
                    tr.expect((d, kind, label), sl)
                    csr.spmm(xd, out=y)
                    got = bits(y)
                    if not same_bits(got, want):
                        rows = sorted(set(np.nonzero(got != want)[0].tolist()))
                        bad.append((d, kind, label, rows, [hex(v) for v in got[rows, 0]], [hex(v) for v in want[rows, 0]]))
    assert not bad, bad


def test_bf16_nan_and_inf_reach_exactly_the_rows_that_reference_them(cuda):
    """three operand rows poisoned with NaN, +inf and -inf in some columns: every output row that references one of them shows it
    in those columns, bit-equal to the model; every other element is bit-equal to the run without the poison"""
    bad = []
    with tuned():
        for name in ("sparse", "dense"):
            mat = graph(name)
            n, ptr, col, val = mat
            for label, (csr, lr) in handles(name, cuda).items():
                for d in (16, 100, 264):
                    clean = x_host(name, "bf16", d).copy()
                    dirty = clean.copy()
                    poison = {5: np.nan, 700: np.inf, n - 2: -np.inf}
                    for r, v in poison.items():
                        dirty[r, 1::3] = v
                    touched = np.zeros((n, d), bool)
                    hit = np.isin(col, list(poison))
                    rows_hit = np.unique(np.repeat(np.arange(n), np.diff(ptr))[hit])
                    assert 0 < len(rows_hit) < n
                    touched[np.ix_(rows_hit, np.arange(1, d, 3))] = True
                    outs = {}
                    for tag, xh in (("clean", clean), ("dirty", dirty)):
                        xd = make_mat("padded", n, d, "bf16", cuda, xh)
                        y = make_mat("padded", n, d, "bf16", cuda)
                        sl = expected_dispatch("bf16", name, xd, y, False)
                        csr.spmm(xd, out=y)
                        outs[tag] = bits(y)
                        want = result_bits(model_sums(mat, xh, sl, lr, False), "bf16")
                        if not same_bits(outs[tag], want):
                            bad.append((name, label, d, tag, n_diff(outs[tag], want)))
                    special = (outs["dirty"] & 0x7f80) == 0x7f80                   # NaN or +-inf
                    if not np.array_equal(special, touched) or not np.array_equal(outs["dirty"][~touched], outs["clean"][~touched]):
                        bad.append((name, label, d, "poison spread", int((special != touched).sum())))
    assert not bad, (len(bad), bad[:10])


# ---- large cases ---------------------------------------------------------------------------------------------------------------
def test_products_shaped_hop_sampled_rows_bit_exact(cuda):
    """The ogbn-products-shaped graph of the bench (test_products_scale_properties' generator) at d = 100: the fp32 default order
    and the bf16 hop on its 128-element pitch (the kernel the published bf16 figures were measured on, which must be
    spmm_bf16_kernel<8, 16, 1, 16>), 4096 sampled rows (the longest included) against the model through rows="""
    from sgl_amd import synthetic
    free, _ = torch.cuda.mem_get_info()
    wl = synthetic.WORKLOADS["S1_products" if free > 60e9 else "S1_small"]
    n, d = wl["n"], wl["d"]
    a_ptr, a_col, a_val = synthetic.chung_lu_torch(n, wl["m"], wl["d_max"], seed=0, device=cuda)
    rowptr, col, val = dev.normalize_adj(a_ptr, a_col, a_val, n, 0.5, None)
    del a_ptr, a_col, a_val
    nnz = col.numel()
    assert nnz / n >= 40
    lr = default_long_row_nnz(nnz)
    csr = dev.DeviceCSR(rowptr, col, val, (n, n))
    rp = rowptr.cpu().numpy()
    deg = np.diff(rp)
    assert csr.info()["n_long_rows"] == int((deg > lr).sum()) > 0
    rows = np.unique(np.concatenate([np.random.default_rng(0).choice(n, 4095, replace=False), [int(deg.argmax())]])).astype(np.int64)
    cc, vv = col.cpu().numpy(), val.cpu().numpy()
    x = synthetic.features_torch(n, d, seed=0, device=cuda)
    rows_d = torch.from_numpy(rows).to(cuda)
    with tuned():
        # fp32, contiguous d = 100: VEC = 4, 25 lanes, one row per step
        y = torch.empty((n, d), device=cuda)
        sl = dispatch("f32", d, ld_of(x), d, x.data_ptr(), y.data_ptr(), False, nnz / n)
        assert [v for _, _, v in sl] == [(4, 64, 1, 16, 0)]
        with Trace("f32") as tr:
            tr.expect("f32", sl)
            csr.spmm(x, out=y)
        want = oracle.oracle_spmm_slots(rp, cc, vv, x.cpu().numpy(), 1, lr, rows=rows)
        got = y[rows_d].cpu().numpy()
        assert same_bits(got.view(np.uint32), want.view(np.uint32)), n_diff(got.view(np.uint32), want.view(np.uint32))
        # bf16 on the 128-element pitch, pad columns zero: the product the operator runs is over the whole pitch
        assert dev.row_pitch(d, elem_size=2) == 128
        xb = torch.zeros((n, 128), dtype=torch.bfloat16, device=cuda)
        xb[:, :d].copy_(x)
        del x, y
        yb = torch.empty((n, 128), dtype=torch.bfloat16, device=cuda)
        sl = dispatch("bf16", 128, 128, 128, xb.data_ptr(), yb.data_ptr(), False, nnz / n)
        assert [v for _, _, v in sl] == [(8, 16, 1, 16)]
        with Trace("bf16") as tr:
            tr.expect("bf16", sl)
            csr.spmm(xb, out=yb)
        assert tr.seen == {(8, 16, 1, 16)}
        want = bits(oracle.oracle_spmm_slots_bf16(rp, cc, vv, xb.cpu(), 4, lr, rows=rows))
        got = bits(yb[rows_d])
        assert same_bits(got, want), n_diff(got, want)
        assert not want[:, d:].any()


def test_bf16_matrix_beyond_2_31_elements(cuda):
    """a bf16 operand of more than 2^31 elements (after test_int64_offsets_beyond_2_31_elements): the gathered rows sit in its
    upper half, at element offsets that do not fit 32 bits; fast and strict order against the model over the rows they read"""
    n_cols, d = 9_000_000, 256
    assert n_cols * d > 2 ** 31
    rows, deg = 4096, 24
    g = torch.Generator(device=cuda).manual_seed(3)
    x = torch.empty((n_cols, d), dtype=torch.bfloat16, device=cuda)
    x.normal_(generator=g)
    hi = torch.randint(n_cols - 100_000, n_cols, (rows, deg - 2), generator=g, device=cuda)
    lo = torch.randint(n_cols // 2 + 1, n_cols // 2 + 1000, (rows, 2), generator=g, device=cuda)
    cols = torch.cat([lo, hi], 1).sort(dim=1).values.to(torch.int32).reshape(-1).contiguous()
    assert int(cols.min()) * d > 2 ** 31 // 2 and int(cols.min()) > n_cols // 2
    vals = torch.rand(rows * deg, generator=g, device=cuda) - 0.5
    rowptr = torch.arange(0, rows + 1, device=cuda, dtype=torch.int64) * deg
    uniq, inv = torch.unique(cols.long(), return_inverse=True)
    x_sub = x[uniq].cpu()                                       # the operand rows that are read, compacted: same terms, same order
    ptr_h, col_h, val_h = rowptr.cpu().numpy(), inv.to(torch.int32).cpu().numpy(), vals.cpu().numpy()
    with tuned():
        for strict in (True, False):
            csr = dev.DeviceCSR(rowptr, cols, vals, (rows, n_cols), strict=strict)
            y = torch.empty((rows, d), dtype=torch.bfloat16, device=cuda)
            sl = dispatch("bf16", d, d, d, x.data_ptr(), y.data_ptr(), strict, float(deg))
            with Trace("bf16") as tr:
                tr.expect(strict, sl)
                csr.spmm(x, out=y)
            if strict:
                want = bits(rne(oracle.oracle_spmm(ptr_h, col_h, val_h, x_sub.float().numpy())))
            else:
                want = bits(oracle.oracle_spmm_slots_bf16(ptr_h, col_h, val_h, x_sub, 64 // sl[0][2][1], default_long_row_nnz(rows * deg)))
            assert same_bits(bits(y), want), (strict, n_diff(bits(y), want))
    del x

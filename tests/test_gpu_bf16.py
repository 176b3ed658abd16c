"""The opt-in bfloat16 hop storage (GraphOp(hop_dtype="bfloat16")) on a real MI355X: run with `-m gpu`.

One definition of rounding everywhere: rne(a) = torch.from_numpy(a).to(torch.bfloat16) on the CPU (round to nearest even).
Bars: strict order bit-exact against the oracle chain with rne after every hop; fast order inside a bound derived from the
reference's own fp32 error and the precision of the format; plans, fused reduction, gathers and models bit-exact against
their definitions over the STORED values."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import oracle
from agg_rows_common import bf16_fast_order_bound, rne
from agg_rows_common import long_row_graph as _long_row_graph
from inputs import hash_matrix
from sgl_amd import _lib, config
from sgl_amd import device as dev

pytestmark = pytest.mark.gpu

D_LIST = [1, 2, 3, 4, 7, 8, 16, 32, 47, 64, 100, 104, 128, 147, 256, 500, 520]
GRAPHS = ["pl2000", "dir40", "sym64", "longrow"]
K = 3


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def bits(t):
    """the 16-bit patterns of a bfloat16 tensor (any device / pitch) as a uint16 array"""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def widened(t):
    return t.detach().cpu().float().numpy()


def long_row_graph(n=1500, seed=5):
    """power-law rows plus three rows of >= 900 non-zeros and some empty ones (canonical CSR, not symmetric); row sums of |a|
    are kept of order 1 so that three hops stay of order 1"""
    return _long_row_graph(n, seed, unit_rows=True)


def matrix(goldens, name):
    """(n, indptr, indices, float32 values) of a normalised golden graph, or of the long-row graph"""
    if name == "longrow":
        a = long_row_graph()
        assert (np.diff(a.indptr) >= 900).sum() == 3 and (np.diff(a.indptr) == 0).sum() > 0
        return a.shape[0], a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float32)
    g = goldens.graph(name)
    n = g.shape[0]
    ptr, col, val = oracle.sym_norm_csr(g.indptr, g.indices, g.data, n, 0.5, None)
    return n, ptr, col, val.astype(np.float32)


def device_csr(ptr, col, val, n, cuda, **kw):
    return dev.DeviceCSR(torch.from_numpy(np.asarray(ptr, np.int64)).to(cuda), torch.from_numpy(np.asarray(col, np.int32)).to(cuda),
                         torch.from_numpy(np.asarray(val, np.float32)).to(cuda), (n, n), **kw)


def device_chain(csr, x, layout, cuda, k=K):
    """[hop 0 .. hop k] as bf16 device [n, d] tensors, hop 0 = rne(x); contiguous or row-padded buffers"""
    n, d = x.shape
    b0 = rne(x)
    if layout == "contig":
        x0 = b0.to(cuda)
        outs = [torch.empty((n, d), dtype=torch.bfloat16, device=cuda) for _ in range(k)]
        csr.spmm_chain(x0, k, outs=outs)
        return [x0] + outs
    x0 = dev.alloc_rows(n, d, cuda, dtype=torch.bfloat16)
    assert x0.stride(0) == dev.row_pitch(d, elem_size=2) and x0.data_ptr() % 16 == 0
    x0.copy_(b0)
    parents = csr.spmm_chain(dev.padded_parent(x0), k)
    for p in parents:                                                  # pad columns are zero and stay zero
        assert p.dtype == torch.bfloat16 and not bits(p[:, d:]).any()
    return [x0] + [p[:, :d] for p in parents]


@pytest.mark.parametrize("gname", GRAPHS)
def test_strict_order_chain_is_bit_exact(goldens, cuda, gname):
    """b_0 = rne(x), b_k = rne(oracle_spmm(b_{k-1}.float())): the fp32 accumulator is bit-equal to the oracle, so no tolerance"""
    n, ptr, col, val = matrix(goldens, gname)
    csr = device_csr(ptr, col, val, n, cuda, strict=True)
    assert csr.info()["n_pieces"] == 0
    bad = []
    for d in D_LIST:
        x = hash_matrix(n, d, seed=d)
        ref = [rne(x)]
        for _ in range(K):
            ref.append(rne(oracle.oracle_spmm(ptr, col, val, ref[-1].float().numpy())))
        for layout in ("contig", "padded"):
            hops = device_chain(csr, x, layout, cuda)
            for k in range(K + 1):
                if not np.array_equal(bits(hops[k]), bits(ref[k])):
                    bad.append((layout, d, k, int((bits(hops[k]) != bits(ref[k])).sum())))
    assert not bad, bad


_FAST_FIGURES = {}


@pytest.mark.parametrize("gname", GRAPHS)
def test_fast_order_per_hop_within_derived_bound(goldens, cuda, gname):
    """Per hop, from the device's own stored hop k-1: T = fp64 product, R = oracle (fp32, strict), G = the device's bf16 hop k,
    b = max(2 max|R - T|, TRUTH_FLOOR max|T|) (truth_report's bound); every element: |G - T| <= 2^-8 |T| + (1 + 2^-8) b.
    RNE to 8 significant bits errs by at most 2^-8 relative; the fp32 sum in another order gets the standing factor 2.
    Recorded on an MI355X (printed, not asserted): worst |G - T| / bound 0.993 ... 0.996; max|hop_3 - truth| / max|truth| against
    the fp64 chain from the unrounded x: pl2000 4.5e-3, dir40 5.5e-3, sym64 5.4e-3, long-row graph 6.8e-3."""
    n, ptr, col, val = matrix(goldens, gname)
    a64 = sp.csr_matrix((val.astype(np.float64), col, ptr), shape=(n, n))
    csr = device_csr(ptr, col, val, n, cuda, strict=False)
    bad, worst, acc_class = [], 0.0, 0.0
    for d in D_LIST:
        x = hash_matrix(n, d, seed=d + 1)
        truth = x.astype(np.float64)
        for _ in range(K):
            truth = a64 @ truth
        for layout in ("contig", "padded"):
            hops = device_chain(csr, x, layout, cuda)
            assert np.array_equal(bits(hops[0]), bits(rne(x)))
            for k in range(1, K + 1):
                xin = widened(hops[k - 1])
                err, bound = bf16_fast_order_bound(a64, ptr, col, val, xin, widened(hops[k]))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                if not (err <= bound).all():
                    bad.append((layout, d, k, float((err - bound).max()), int((err > bound).sum())))
            # the accuracy class of the whole chain against the fp64 truth from the UNROUNDED x: recorded, not asserted
            acc_class = max(acc_class, float(np.abs(widened(hops[K]) - truth).max() / np.abs(truth).max()))
    _FAST_FIGURES[gname] = acc_class
    print(f"bf16 fast order on {gname}: worst |G - T| / bound = {worst:.4f}; max|hop_{K} - truth| / max|truth| = {acc_class:.3e}")
    assert not bad, bad


@pytest.mark.parametrize("gname", ["pl2000", "longrow"])
def test_fast_order_is_plan_independent(goldens, cuda, gname):
    """same bits from the default plan, 64-nnz items, no XCD remap, and a random row permutation behind a row map"""
    n, ptr, col, val = matrix(goldens, gname)
    base = device_csr(ptr, col, val, n, cuda)
    if gname == "longrow":
        assert base.info()["n_pieces"] >= 3
    perm = torch.from_numpy(np.random.default_rng(7).permutation(n).astype(np.int32)).to(cuda)
    p_ptr, p_col, p_val = dev.permute_rows(base.rowptr, base.col, base.val, perm)
    mapped = dev.DeviceCSR(p_ptr, p_col, p_val, (n, n)).set_rowmap(perm)
    others = {"item_nnz=64": device_csr(ptr, col, val, n, cuda, item_nnz=64),
              "xcd_remap=False": device_csr(ptr, col, val, n, cuda, xcd_remap=False), "rowmap": mapped}
    for d in (8, 16, 100, 104, 128, 147, 520):
        x = hash_matrix(n, d, seed=d + 2)
        for layout in ("contig", "padded"):
            want = [bits(h) for h in device_chain(base, x, layout, cuda)]
            for name, csr in others.items():
                got = [bits(h) for h in device_chain(csr, x, layout, cuda)]
                for k in range(K + 1):
                    assert np.array_equal(got[k], want[k]), (name, layout, d, k)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("d", [100, 37])
def test_fused_reduce_equals_reduce_over_stored_hops(goldens, cuda, strict, d):
    from sgl_amd.operators.graph_op import LaplacianGraphOp
    adj = goldens.graph("pl2000")
    x = hash_matrix(adj.shape[0], d, seed=21)
    op = LaplacianGraphOp(K, r=0.5, hop_dtype="bfloat16", strict_order=strict)
    hops = op.propagate(adj, x)
    wide = [h.float() for h in hops]
    w = torch.tensor([0.5, 0.25, 0.15, 0.1])
    cases = [("sum", _lib.SGL_REDUCE_SUM, {}), ("mean", _lib.SGL_REDUCE_MEAN, {"divisor": K + 1}), ("max", _lib.SGL_REDUCE_MAX, {}),
             ("min", _lib.SGL_REDUCE_MIN, {}), ("wsum", _lib.SGL_REDUCE_WSUM, {"weights": w})]
    for kind, code, kw in cases:
        fused = op.propagate_reduce(adj, x, kind, start=0, end=K + 1, **kw)
        assert fused.dtype == torch.float32 and fused.shape == (adj.shape[0], d)
        want = dev.hop_reduce(code, wide, w if kind == "wsum" else None)
        assert np.array_equal(fused.cpu().numpy(), want.cpu().numpy()), (kind, strict, d)
    last = op.propagate_reduce(adj, x, "last")
    assert last.dtype == torch.bfloat16 and np.array_equal(bits(last), bits(hops[K]))


@pytest.mark.parametrize("d", [100, 147])
def test_gathers_widen_exactly(cuda, d):
    n, H = 3000, 4
    rng = np.random.default_rng(d)
    hops = []
    for h in range(H):
        t = dev.alloc_rows(n, d, cuda, dtype=torch.bfloat16)
        t.copy_(rne(hash_matrix(n, d, seed=30 + h)))
        hops.append(t)
    idx = np.concatenate([rng.integers(0, n, 777), [5, 5, 5, n - 1, 0, -1, -n]]).astype(np.int64)     # repeated, unsorted, negative
    for index in (idx, torch.from_numpy(idx).to(cuda), list(idx)):
        many = dev.gather_hops(hops, index)
        for h in range(H):
            one = dev.gather_rows(hops[h], index)
            want = widened(hops[h])[idx]
            for got in (many[h], one):
                assert got.dtype == torch.float32 and got.shape == (len(idx), d) and got.is_cuda
                assert np.array_equal(got.cpu().numpy(), want)
                pad = dev.own_pad(got)
                assert pad == dev.row_pitch(d) - d
                if pad:
                    assert not dev.padded_parent(got)[:, d:].cpu().numpy().any()
    # contiguous (unpadded) bf16 source, caller's output, a single index
    src = hops[0].contiguous()
    out = torch.full((len(idx), d), 7.0, dtype=torch.float32, device=cuda)
    dev.gather_rows(src, idx, out=out)
    assert np.array_equal(out.cpu().numpy(), widened(hops[0])[idx])
    assert np.array_equal(dev.gather_rows(hops[1], [17]).cpu().numpy(), widened(hops[1])[[17]])
    with pytest.raises(IndexError):
        dev.gather_rows(hops[0], [n])


def _strict_reference(adj, x, r=0.5, alpha=None):
    n = adj.shape[0]
    ptr, col, val = oracle.sym_norm_csr(adj.indptr, adj.indices, adj.data, n, r, alpha)
    val = val.astype(np.float32)
    ref = [rne(x)]
    for _ in range(K):
        ref.append(rne(oracle.oracle_spmm(ptr, col, val, ref[-1].float().numpy())))
    return ref


@pytest.mark.parametrize("kind", ["laplacian", "ppr"])
def test_operator_api(goldens, cuda, kind, monkeypatch, tmp_path):
    from sgl_amd.operators.graph_op import LaplacianGraphOp, PprGraphOp

    def make(**kw):
        return LaplacianGraphOp(K, r=0.5, **kw) if kind == "laplacian" else PprGraphOp(K, r=0.5, alpha=0.15, **kw)
    alpha = None if kind == "laplacian" else 0.15
    adj = goldens.graph("pl2000")
    n, d = adj.shape[0], 100
    x = hash_matrix(n, d, seed=40)
    fp32_before = [h.cpu().numpy() for h in make().propagate(adj, x)]

    # strict order: K + 1 CUDA bf16 [n, d] matrices at the documented pitch, bit-equal to the oracle chain
    hops = make(hop_dtype="bfloat16", strict_order=True).propagate(adj, x)
    ref = _strict_reference(adj, x, alpha=alpha)
    assert len(hops) == K + 1
    for k, h in enumerate(hops):
        assert h.is_cuda and h.dtype == torch.bfloat16 and h.shape == (n, d) and h.stride() == (dev.row_pitch(d, elem_size=2), 1)
        assert h.data_ptr() % 16 == 0 and not bits(dev.padded_parent(h)[:, d:]).any()
        assert np.array_equal(bits(h), bits(ref[k])), k

    # a device tensor as input: hop 0 is a rounded COPY, the caller's x is neither modified nor aliased
    xt = torch.from_numpy(x).to(cuda)
    keep = xt.clone()
    fast = make(hop_dtype="bfloat16").propagate(adj, xt)
    assert torch.equal(xt, keep) and xt.dtype == torch.float32
    assert fast[0].dtype == torch.bfloat16 and fast[0].untyped_storage().data_ptr() != xt.untyped_storage().data_ptr()
    assert np.array_equal(bits(fast[0]), bits(rne(x)))
    # reorder="community": same bits as without it
    reordered = make(hop_dtype="bfloat16", reorder="community").propagate(adj, xt)
    for k in range(K + 1):
        assert np.array_equal(bits(reordered[k]), bits(fast[k])), k
    # cache_adj: the second call of one operator re-uses its adjacency and gives the same bits
    op = make(hop_dtype="bfloat16", cache_adj=True)
    first = [bits(h) for h in op.propagate(adj, x)]
    assert all(np.array_equal(a, bits(b)) for a, b in zip(first, op.propagate(adj, x)))
    assert all(np.array_equal(a, bits(b)) for a, b in zip(first, fast))

    # options it does not combine with
    for other in ("host_output", "slab_hops"):
        with pytest.raises(ValueError, match=other):
            make(hop_dtype="bfloat16", **{other: True}).propagate(adj, x)
    with pytest.raises(ValueError):
        make(hop_dtype="float16").propagate(adj, x)

    # config.hop_dtype is the default of the ctor argument
    monkeypatch.setattr(config, "hop_dtype", "bfloat16")
    via_config = make().propagate(adj, x)
    assert all(h.dtype == torch.bfloat16 for h in via_config) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(via_config, fast))
    assert all(h.dtype == torch.float32 for h in make(hop_dtype="float32").propagate(adj, x))
    monkeypatch.setattr(config, "hop_dtype", "float32")

    # caches never mix precisions: the shared hop store and the on-disk cache hold float32 only
    monkeypatch.setattr(config, "share_hops", True)
    shared32 = make().propagate(adj, x)
    shared16 = make(hop_dtype="bfloat16").propagate(adj, x)
    again32 = make().propagate(adj, x)
    assert all(h.dtype == torch.bfloat16 for h in shared16) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(shared16, fast))
    assert all(h.dtype == torch.float32 for h in shared32 + again32)
    monkeypatch.setattr(config, "share_hops", False)
    cached16 = make(hop_dtype="bfloat16", hop_cache_dir=str(tmp_path)).propagate(adj, x)
    assert all(h.dtype == torch.bfloat16 for h in cached16) and not list(tmp_path.iterdir())

    # an fp32 operator on the same adjacency afterwards: bit-identical fp32 hops
    fp32_after = make().propagate(adj, x)
    for k in range(K + 1):
        assert fp32_after[k].dtype == torch.float32 and np.array_equal(fp32_after[k].cpu().numpy(), fp32_before[k]), k


def test_device_layer_refusals(goldens, cuda):
    n, ptr, col, val = matrix(goldens, "sym64")
    csr = device_csr(ptr, col, val, n, cuda)
    xb = rne(hash_matrix(n, 8, seed=1)).to(cuda)
    xf = xb.float()
    with pytest.raises(TypeError):
        csr.spmm(xb, out=torch.empty_like(xf))                     # mixed X / Y dtype
    with pytest.raises(TypeError):
        csr.spmm_chain(xf, 1, outs=[torch.empty_like(xb)])
    with pytest.raises(TypeError):
        csr.capture_chain(xb, [torch.empty_like(xb)])
    with pytest.raises(TypeError):
        csr.spmm_multi(xb, [0], 8)
    with pytest.raises(TypeError):
        csr.spmm_axpb_clamp(xb, 0.5)
    from sgl_amd.dist import ShardedGraphOp
    with pytest.raises(TypeError):                                  # the multi-GPU layouts have no bfloat16 form: no such argument
        ShardedGraphOp(2, hop_dtype="bfloat16")
    # full-matrix aggregators: widened hop by hop, then the fp32 kernels
    hops = [rne(hash_matrix(n, 8, seed=s)).to(cuda) for s in (2, 3)]
    got = dev.hop_reduce(_lib.SGL_REDUCE_SUM, hops)
    want = dev.hop_reduce(_lib.SGL_REDUCE_SUM, [h.float() for h in hops])
    assert got.dtype == torch.float32 and torch.equal(got, want)


@pytest.mark.parametrize("name", ["SGC", "GAMLP"])
def test_models_see_only_the_stored_values(goldens, cuda, name, monkeypatch):
    """logits under bf16 storage == logits of the same model (same seed) fed the widened copies of the same hops"""
    from sgl_amd.models.homo import GAMLP, SGC
    adj = goldens.graph("pl2000")
    n, d, classes = adj.shape[0], 100, 7
    x = hash_matrix(n, d, seed=50)
    idx = [int(i) for i in np.random.default_rng(3).integers(0, n, 300)]

    def build():
        torch.manual_seed(1234)
        m = SGC(K, d, classes) if name == "SGC" else GAMLP(K, d, classes, 64, 2)
        return m.to(cuda).eval()
    monkeypatch.setattr(config, "hop_dtype", "bfloat16")
    model = build()
    model.preprocess(adj, x)
    hops = model._pre_graph_op.propagate(adj, x)
    assert all(h.dtype == torch.bfloat16 for h in hops)
    if name == "SGC":
        assert model.hops_available() != "kept"                    # folded into the propagation
        assert model._processed_feature.dtype == torch.bfloat16
    else:
        assert all(h.dtype == torch.bfloat16 for h in model._processed_feat_list)
    with torch.no_grad():
        got = model.model_forward(idx, cuda)
    monkeypatch.setattr(config, "hop_dtype", "float32")
    ref = build()
    wide = [h.float() for h in hops]
    ref._pre_msg_learnable = model._pre_msg_learnable
    ref._processed_feat_list = wide
    if not ref._pre_msg_learnable:
        ref._processed_feature = ref._pre_msg_op.aggregate(wide)
    with torch.no_grad():
        want = ref.model_forward(idx, cuda)
    assert got.dtype == torch.float32 and got.shape == (len(idx), classes)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())

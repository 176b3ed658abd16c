"""Every dense-matrix entry point of the library with rows whose element offset does not fit in 32 bits, on a real MI355X: run
with `-m gpu`.

The contract shape of the project is one rank of ogbn-papers100M, hop matrices of 14.2 G elements: a kernel that forms
`row * pitch` in 32 bits passes every small test and fails there.  Every entry point takes its pitch as an int64, so a far row
needs a large PITCH, not many rows (far_common.py): one flat table of a little over 2^32 float32 elements (tier A; 2^31 at tier B)
is viewed as [n, ld] with (n - 1) * ld beyond the threshold, and every matrix argument of a call -- hops, outputs, residual,
accumulator, centres, gradients, the small [n, H] score matrices -- is a column range of that view.  The kernels touch n x d
values; the table is filled once with a NaN pattern, so a wrapped read returns NaN or another row's hashed values and a wrapped
write leaves NaN where the result is expected.

Per entry point, the PRIMARY check is the reference its own test uses (float64 / the oracle / a float32 statement, with that test's
constants: none is chosen here).  SECONDARY: the same call on ordinary alloc_rows buffers holding the same values gives the same
bits -- no kernel chooses its arithmetic by where a row lives.  After every test its views are re-filled and the whole table is
swept: every 32-bit word must hold the fill again.

test_true_size_contiguous covers what a pitch cannot: a flat element index or a `row * d` of a contiguous fast path, with
genuinely contiguous matrices of just over 2^31 elements, sampled rows against numpy.

Before the first run the index arithmetic of every kernel launched here was read (sgl_aggregate.hip, sgl_aggregate_bf16.hip,
sgl_spmm.hip, sgl_spmm_bf16.hip, sgl_spmm_common.h, sgl_rows.h, sgl_edge.hip, sgl_kmeans.hip and their launchers): rows, gathered
indices and pitches are int64 everywhere; the one 32-bit pitch, hop_lincomb's ldw, is capped by its entry point, so its weight
matrix stays near here."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import edge_scores_common as esc
import kmeans_common as kc
import oracle
from agg_rows_common import PARITY_TOL as TOL
from agg_rows_common import (BIAS, bf16_fast_order_bound, gate_reference, long_row_graph, recursive_step_by_step, reduce_statement, rne,
                             same_bits32, sig_mix, t32, t64, vector)
from far_common import FILL32, GIB, TIERS, FarTable, default_pitch_rows, pick_tier, table_elems
from inputs import hash_matrix
from sgl_amd import _lib, synthetic
from sgl_amd import device as dev

pytestmark = pytest.mark.gpu

N = 515                       # row kernels: several workgroups for every lanes-per-row setting, plus a tail
WIDTHS = (104, 147)           # the widest vector path (float32 4-float lanes, bfloat16 BV = 8) / a width that cannot take it
HOPS = (4, 11)
NAN = float("nan")
OPS = {"sum": _lib.SGL_REDUCE_SUM, "mean": _lib.SGL_REDUCE_MEAN, "max": _lib.SGL_REDUCE_MAX, "min": _lib.SGL_REDUCE_MIN,
       "wsum": _lib.SGL_REDUCE_WSUM}


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def far(cuda):
    """the one table of the module, NaN-filled once"""
    torch.cuda.empty_cache()                             # what earlier modules left in torch's cache counts as free
    free, _ = torch.cuda.mem_get_info()
    tier = pick_tier(free)
    if tier is None:
        pytest.skip(f"far-offset tests need {TIERS['B'][0] / GIB:.0f} GiB of free device memory, {free / GIB:.1f} GiB are free")
    flat = torch.empty(table_elems(tier), dtype=torch.float32, device=cuda)
    flat.view(torch.int32).fill_(FILL32)
    print(f"\n[far offsets] tier {tier}: rows beyond {TIERS[tier][1]} elements, table of {flat.numel() * 4 / 1e9:.1f} GB, "
          f"{free / GIB:.1f} GiB were free")
    table = FarTable(flat, TIERS[tier][1])
    table.tier = tier
    yield table
    del table.flat, flat
    torch.cuda.empty_cache()


def stray_words(table):
    """32-bit words of the table that do not hold the fill: one read of the table, in chunks"""
    words = table.flat.view(torch.int32)
    bad = torch.zeros((), dtype=torch.int64, device=words.device)
    step = 1 << 28
    for lo in range(0, words.numel(), step):
        bad += torch.count_nonzero(words[lo:lo + step] != FILL32)
    return int(bad)


class Far:
    """the buffers of one run as views of the table"""

    def __init__(self, lay, fam):
        self.lay, self.fam = lay, fam

    def out(self, m, d, dtype=torch.float32, step=1):
        v = self.lay.take(d, dtype, rows=m, step=step)
        self.fam.far_rows += v.far_rows(self.lay.table.threshold)
        self.fam.half_rows += v.far_rows(1 << 31)
        self.fam.views += 1
        return v.t

    def inp(self, host, step=1):
        host = host if torch.is_tensor(host) else torch.from_numpy(np.ascontiguousarray(host))
        t = self.out(host.shape[0], host.shape[1], host.dtype, step)
        t.copy_(host)
        return t


class Near:
    """the same buffers as ordinary alloc_rows matrices, pad columns and outputs holding the same fill"""

    def __init__(self, device):
        self.device = device

    def out(self, m, d, dtype=torch.float32, step=1):
        t = dev.alloc_rows(m, d, self.device, zero_pad=False, dtype=dtype)
        parent = dev.padded_parent(t)
        if dtype == torch.float32:
            parent.view(torch.int32).fill_(FILL32)
        else:
            parent.view(torch.int16).fill_(FILL32 & 0xFFFF)
        return t

    def inp(self, host, step=1):
        host = host if torch.is_tensor(host) else torch.from_numpy(np.ascontiguousarray(host))
        t = self.out(host.shape[0], host.shape[1], host.dtype)
        t.copy_(host)
        return t


class Family:
    def __init__(self, table, name, n, cuda, pitch_rows=None):
        self.table, self.name, self.n, self.cuda = table, name, n, cuda
        self.lay = table.layout(n, pitch_rows or default_pitch_rows(n))      # several rows beyond the threshold, not one
        self.far_rows = self.half_rows = self.views = self.calls = 0

    def both(self, body, where=None):
        """body(*factories) -> {name: tensor}: once with the table's views (where: one letter per factory, "f" = far, "n" = near;
        default all far), once with near buffers only.  Returns the far run's results on the CPU; the near run's must have the
        same bits (SECONDARY check: the comparison with the reference is the caller's, on what is returned)."""
        k = body.__code__.co_argcount
        where = where or "f" * k
        near = Near(self.cuda)
        got = {key: t.detach().to("cpu", copy=True) for key, t in body(*[Far(self.lay, self) if w == "f" else near for w in where]).items()}
        self.lay.refill()                                                  # (the copies to the CPU above have synchronised)
        same = {key: t.detach().cpu() for key, t in body(*[near] * k).items()}
        for key in got:
            assert raw_equal(got[key], same[key]), (self.name, key, "far and near buffers give different bits")
        self.calls += 1
        return got


def raw_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    kind = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(kind), b.contiguous().view(kind))


@contextlib.contextmanager
def family(table, name, n, cuda, pitch_rows=None):
    fam = Family(table, name, n, cuda, pitch_rows)
    try:
        yield fam
    finally:
        fam.lay.refill()
    stray = stray_words(table)
    print(f"\n[far {name}] tier {table.tier}, n = {n}, pitch {fam.lay.ld}: {fam.calls} far calls over {fam.views} far matrices, "
          f"{fam.far_rows} rows beyond {table.threshold} elements ({fam.half_rows} beyond 2^31); words off the fill afterwards: {stray}")
    assert fam.far_rows > 0 and fam.calls > 0
    assert stray == 0


def call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()), name)


def ld(t):
    return t.stride(0)


def P(t):
    return None if t is None else _lib.ptr(t)


def np32(t):
    return t.float().numpy() if t.dtype == torch.bfloat16 else t.numpy()


def bits16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


_HOPS = {}


def hops_host(n, d, H, seed=0):
    """[hash_matrix scaled by (1 - 0.04 h)]: distinct from row to row and hop to hop; built once per shape and left unchanged"""
    have = _HOPS.setdefault((n, d, seed), [])
    for h in range(len(have), H):
        have.append(np.ascontiguousarray((hash_matrix(n, d, seed=7000 + 100 * seed + 31 * d + h) * np.float32(1.0 - 0.04 * h)).astype(np.float32)))
    return have[:H]


def truth_ok(got, ref32, truth, cond=None):
    rep = oracle.truth_report(np.asarray(got), np.asarray(ref32), np.asarray(truth), cond=None if cond is None else np.asarray(cond))
    return rep["ok"] and bool(np.isfinite(np.asarray(got)).all())


# ---- the smallest true-size case (first: it runs before the table is allocated) -------------------------------------------------------
TRUE_N, TRUE_D = 16_777_300, 128                  # just over 2^31 elements: 8.6 GB per float32 matrix, 4.3 GB per bfloat16 one
TRUE_NEEDS = 45 * GIB


def test_true_size_contiguous(cuda):
    """Genuinely contiguous [16 777 300, 128] matrices: what a large pitch cannot catch -- a 32-bit FLAT element index, or a
    contiguous fast path that forms row * d.  sgl_hop_reduce_f32 (sum, max) and sgl_hop_concat_f32 with H = 2, sgl_hop_reduce_bf16_f32,
    sgl_hop_concat_bf16, sgl_col_signature_f32, sgl_hop_colsum_f32, sgl_gather_rows_padded_f32 and sgl_scatter_rows_f32 with indices at
    both ends; the first 5, the last 5 and 200 drawn rows (read back with torch indexing) against numpy, the signature against a
    chunked uint64 torch reduction over all rows.

    The column sums use weights that are zero except at the sampled rows and at the 84 rows that start beyond 2^31 elements, so
    that a row read from a wrapped place moves the result by about 1 / 300 of its magnitude; the reference is the float64 sum over
    those rows, under the bar of test_hop_colsum_is_the_weight_gradient_of_the_row_dots: 2e-6 of sum |w x|."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < TRUE_NEEDS:
        pytest.skip(f"the true-size case needs {TRUE_NEEDS / GIB:.0f} GiB of free device memory, {free / GIB:.1f} GiB are free")
    n, d = TRUE_N, TRUE_D
    first_far = -(-2 ** 31 // d)                                                # the first row that starts beyond 2^31 elements
    assert n * d > 2 ** 31 and n - first_far == 84
    feats = []
    for h in range(2):
        t = torch.empty((n, d), dtype=torch.float32, device=cuda)
        synthetic.hashed_features_torch(5 + h, 0, n, d, device=cuda, out=t)
        feats.append(t)
    rows = np.concatenate([np.arange(0, 5), np.arange(n - 5, n), np.random.default_rng(0).integers(0, n, 200)])
    idx = torch.from_numpy(rows).to(cuda)
    host = [f[idx].cpu().numpy() for f in feats]
    assert all(np.abs(h).max() > 0 and len(np.unique(h[:, 0])) > 200 for h in host)          # hashed values, distinct from row to row
    print(f"\n[far true size] 2 x [{n}, {d}] float32 ({n * d * 4 / 1e9:.1f} GB each), {len(rows)} sampled rows, "
          f"{int((rows >= first_far).sum())} of them beyond 2^31 elements; {free / GIB:.1f} GiB were free")

    y = dev.hop_reduce(_lib.SGL_REDUCE_SUM, feats)
    assert np.array_equal(y[idx].cpu().numpy(), (np.float32(0) + host[0]) + host[1])
    del y
    y = dev.hop_reduce(_lib.SGL_REDUCE_MAX, feats)
    assert np.array_equal(y[idx].cpu().numpy(), np.maximum(host[0], host[1]))
    del y
    y = torch.empty((n, 2 * d), dtype=torch.float32, device=cuda)
    ptrs, lds = _lib.hop_arrays(feats)
    call("sgl_hop_concat_f32", 2, ptrs, lds, P(y), 2 * d, n, d)
    assert np.array_equal(y[idx].cpu().numpy(), np.hstack(host))
    del y

    # the column signature over all rows, against a chunked torch reduction
    sig = dev.column_signature(feats[0])
    want_sig = torch.zeros(d, dtype=torch.int64, device=cuda)
    step = 1 << 20
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        want_sig += mix_torch(feats[0][lo:hi].view(torch.int32), torch.arange(lo, hi, device=cuda).view(-1, 1)).sum(0)
    assert sig is not None and torch.equal(sig, want_sig)
    del want_sig

    # weighted column sums: weights at the sampled rows and at every row beyond 2^31 elements, zero elsewhere
    wrows = np.unique(np.concatenate([rows, np.arange(first_far, n)]))
    wvals = hash_matrix(len(wrows), 1, seed=9)[:, 0]
    w = torch.zeros(n, dtype=torch.float32, device=cuda)
    widx = torch.from_numpy(wrows).to(cuda)
    w[widx] = torch.from_numpy(wvals).to(cuda)
    got = dev.hop_colsum(feats, w, shared=True).cpu().numpy().astype(np.float64)
    for h in range(2):
        terms = feats[h][widx].cpu().numpy().astype(np.float64) * wvals.astype(np.float64)[:, None]
        assert float((np.abs(got[h] - terms.sum(0)) / np.maximum(np.abs(terms).sum(0), 1e-30)).max()) <= 2e-6, h
    del w

    # row gather / scatter with indices at both ends
    m = len(rows)
    out = torch.full((m, d), NAN, dtype=torch.float32, device=cuda)
    call("sgl_gather_rows_padded_f32", P(feats[1]), d, n, P(idx), m, P(out), d, d, 0)
    assert np.array_equal(out.cpu().numpy(), host[1])
    dst_rows = np.concatenate([np.arange(0, 5), np.arange(n - 5, n), np.random.default_rng(1).choice(n - 10, 200, replace=False) + 5])
    dst = torch.from_numpy(dst_rows).to(cuda)
    dev.scatter_rows(feats[1], idx, dst, feats[0])                               # feats[0] is overwritten at the drawn rows
    assert np.array_equal(feats[0][dst].cpu().numpy(), host[1])
    del feats, out

    hops16 = []
    for h in range(2):
        t = torch.empty((n, d), dtype=torch.float32, device=cuda)
        synthetic.hashed_features_torch(15 + h, 0, n, d, device=cuda, out=t)
        hops16.append(t.to(torch.bfloat16))
        del t
    host16 = [f[idx].cpu() for f in hops16]
    wide = [h.float().numpy() for h in host16]
    for kind in ("sum", "max"):
        y = dev.hop_reduce(OPS[kind], hops16)
        assert y.dtype == torch.float32 and same_bits32(y[idx].cpu().numpy(), reduce_statement(kind, wide, None)), kind
        del y
    y = dev.hop_concat(hops16, out_dtype=torch.bfloat16)
    assert y.dtype == torch.bfloat16 and np.array_equal(bits16(y[idx].cpu()), bits16(torch.cat(host16, dim=1)))
    del y, hops16
    torch.cuda.empty_cache()


# ---- SpMM float32 -------------------------------------------------------------------------------------------------------------------
_GRAPH = {}


def graph(kind):
    if kind not in _GRAPH:
        a = long_row_graph(unit_rows=(kind == "bf16"))
        assert a.shape[0] == 1500 and (np.diff(a.indptr) >= 900).sum() == 3
        _GRAPH[kind] = (a.shape[0], a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float32))
    return _GRAPH[kind]


def device_csr(kind, cuda, strict):
    n, ptr, col, val = graph(kind)
    csr = dev.DeviceCSR(torch.from_numpy(ptr).to(cuda), torch.from_numpy(col).to(cuda), torch.from_numpy(val).to(cuda), (n, n), strict=strict)
    info = csr.info()
    assert info["n_pieces"] == 0 if strict else (info["n_long_rows"] >= 3 and info["n_pieces"] >= 3)     # split rows + fix-up kernel
    return csr


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_spmm_f32(cuda, far, strict):
    """sgl_spmm_f32 on the long-row graph, both values of accumulate, with X far, Y far, and both: strict order bit-equal to the
    oracle, fast order as test_spmm_fuzz_random_shapes compares it"""
    n, ptr, col, val = graph("f32")
    csr = device_csr("f32", cuda, strict)
    with family(far, f"spmm_f32 {'strict' if strict else 'fast'}", n, cuda) as fam:
        for d in WIDTHS:
            x, y0 = hash_matrix(n, d, seed=11 + d), hash_matrix(n, d, seed=12 + d)
            scale = oracle.oracle_spmm(ptr, col, np.abs(val), np.abs(x))
            for where in ("fn", "nf", "ff"):
                for accumulate in (False, True):
                    ref = oracle.oracle_spmm(ptr, col, val, x, out=y0.copy()) if accumulate else oracle.oracle_spmm(ptr, col, val, x)

                    def body(bx, by):
                        y = by.inp(y0) if accumulate else by.out(n, d)
                        csr.spmm(bx.inp(x), out=y, accumulate=accumulate)
                        return {"y": y}
                    y = fam.both(body, where)["y"].numpy()
                    ctx = (d, where, accumulate)
                    if strict:
                        assert np.array_equal(y, ref), ctx
                    elif accumulate:
                        assert oracle.parity_ok(y, ref, TOL), ctx
                    else:
                        rep = oracle.parity_report(y, ref, TOL, scale=scale)
                        assert rep["ok"], (ctx, rep)


def acc_statement(mode, acc0, y, w, divisor):
    """sgl_spmm_acc's update in numpy float32: add / rounded product then add / NaN-propagating max, min; then one true division"""
    with np.errstate(all="ignore"):
        if mode == 0:
            acc = acc0 + y
        elif mode == 1:
            acc = acc0 + np.float32(w) * y
        else:
            acc = (np.maximum if mode == 2 else np.minimum)(acc0, y)
        return (acc / np.float32(divisor)).astype(np.float32) if (mode < 2 and divisor != 1.0) else acc.astype(np.float32)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_spmm_f32_chain_and_epilogues(cuda, far, strict):
    """sgl_spmm_chain_f32 (k = 3, every hop far), sgl_spmm_axpb_clamp_f32 with a far residual, sgl_spmm_acc_f32 in each mode with a
    far ACC: as test_spmm_chain_equals_repeated_spmm, test_spmm_axpb_clamp_epilogue and the epilogue's float32 statement state them"""
    n, ptr, col, val = graph("f32")
    csr = device_csr("f32", cuda, strict)
    with family(far, f"spmm_f32 chain / axpb_clamp / acc {'strict' if strict else 'fast'}", n, cuda) as fam:
        for d in WIDTHS:
            x, res = hash_matrix(n, d, seed=13 + d), hash_matrix(n, d, seed=14 + d)

            def chain(b):
                outs = [b.out(n, d) for _ in range(3)]
                csr.spmm_chain(b.inp(x), 3, outs=outs)
                return {f"hop{k + 1}": o for k, o in enumerate(outs)}
            got = fam.both(chain)
            prev = x
            for k in range(1, 4):
                y = got[f"hop{k}"].numpy()
                ref = oracle.oracle_spmm(ptr, col, val, prev)
                if strict:
                    assert np.array_equal(y, ref), (d, k)
                else:
                    rep = oracle.parity_report(y, ref, TOL, scale=oracle.oracle_spmm(ptr, col, np.abs(val), np.abs(prev)))
                    assert rep["ok"], (d, k, rep)
                prev = y

            ax = oracle.oracle_spmm(ptr, col, val, x)

            def clamp(b):
                y = b.out(n, d)
                csr.spmm_axpb_clamp(b.inp(x), 0.8, b.inp(res), -0.5, 0.75, out=y)
                return {"y": y}
            y = fam.both(clamp)["y"].numpy()
            ref = np.clip((np.float32(0.8) * ax + res).astype(np.float32), np.float32(-0.5), np.float32(0.75))
            if strict:
                assert np.array_equal(y, ref), d
            else:
                pre = np.abs(np.float32(0.8) * ax + res).max()
                assert np.abs(y - ref).max() <= TOL * pre and y.min() >= -0.5 and y.max() <= 0.75, d

            acc0 = hash_matrix(n, d, seed=15 + d)
            scale = oracle.oracle_spmm(ptr, col, np.abs(val), np.abs(x))
            for mode, w, divisor in ((0, 1.0, 1.0), (0, 1.0, 4.0), (1, 0.3, 1.0), (1, -1.5, 3.0), (2, 1.0, 1.0), (3, 1.0, 1.0)):
                def acc(b):
                    xd, y, a = b.inp(x), b.out(n, d), b.inp(acc0)
                    call("sgl_spmm_acc_f32", csr._h, P(xd), ld(xd), P(y), ld(y), d, P(a), ld(a), w, mode, divisor)
                    return {"y": y, "acc": a}
                got = fam.both(acc)
                y = got["y"].numpy()
                if strict:
                    assert np.array_equal(y, ax), (d, mode)
                else:
                    assert oracle.parity_report(y, ax, TOL, scale=scale)["ok"], (d, mode)
                assert same_bits32(got["acc"].numpy(), acc_statement(mode, acc0, y, w, divisor)), (d, mode, w, divisor)


# ---- SpMM bfloat16 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_spmm_bf16(cuda, far, strict):
    """sgl_spmm_bf16, sgl_spmm_chain_bf16 (k = 3) and sgl_spmm_acc_bf16 with every matrix far: strict order bit-equal to the
    rne(oracle_spmm(...)) chain of test_gpu_bf16.py, fast order inside the bound of test_fast_order_per_hop_within_derived_bound;
    the aggregate is the float32 statement over the ROUNDED product widened again"""
    n, ptr, col, val = graph("bf16")
    a64 = sp.csr_matrix((val.astype(np.float64), col, ptr), shape=(n, n))
    csr = device_csr("bf16", cuda, strict)
    with family(far, f"spmm_bf16 {'strict' if strict else 'fast'}", n, cuda) as fam:
        for d in WIDTHS:
            b0 = rne(hash_matrix(n, d, seed=d))

            def check(tag, xin, y):
                if strict:
                    assert np.array_equal(bits16(y), bits16(rne(oracle.oracle_spmm(ptr, col, val, xin.float().numpy())))), (d, tag)
                else:
                    err, bound = bf16_fast_order_bound(a64, ptr, col, val, xin.float().numpy(), y.float().numpy())
                    assert (err <= bound).all(), (d, tag, int((err > bound).sum()))

            def one(b):
                y = b.out(n, d, torch.bfloat16)
                csr.spmm(b.inp(b0), out=y)
                return {"y": y}
            check("spmm", b0, fam.both(one)["y"])

            def chain(b):
                outs = [b.out(n, d, torch.bfloat16) for _ in range(3)]
                csr.spmm_chain(b.inp(b0), 3, outs=outs)
                return {f"hop{k + 1}": o for k, o in enumerate(outs)}
            got = fam.both(chain)
            prev = b0
            for k in range(1, 4):
                check(f"chain hop {k}", prev, got[f"hop{k}"])
                prev = got[f"hop{k}"]

            acc0 = hash_matrix(n, d, seed=16 + d)
            for mode, w, divisor in ((0, 1.0, 4.0), (1, -1.5, 1.0), (2, 1.0, 1.0), (3, 1.0, 1.0)):
                def acc(b):
                    y, a = b.out(n, d, torch.bfloat16), b.inp(acc0)
                    csr.spmm_acc(b.inp(b0), y, a, w=w, divisor=divisor, mode={0: "sum", 1: "wsum", 2: "max", 3: "min"}[mode])
                    return {"y": y, "acc": a}
                got = fam.both(acc)
                check(f"acc mode {mode}", b0, got["y"])
                assert same_bits32(got["acc"].numpy(), acc_statement(mode, acc0, got["y"].float().numpy(), w, divisor)), (d, mode)


# ---- gathers and scatter --------------------------------------------------------------------------------------------------------------
def index_list(n):
    """n indices: the first rows, the last rows, repeats, negatives, then seeded draws"""
    head = np.concatenate([np.arange(10), np.arange(n - 10, n), [5, 5, 5, n - 1, n - 1], [-1, -2, -n, 1 - n, -n // 2]]).astype(np.int64)
    rest = np.random.default_rng(n).integers(-n, n, n - len(head))
    return np.concatenate([head, rest]).astype(np.int64)


def test_gathers_and_scatter(cuda, far):
    """sgl_gather_rows_f32, sgl_gather_rows_padded_f32 (C ABI and dev.gather_rows(out=)), sgl_gather_hops_padded_f32 with 4 hops,
    sgl_scatter_rows_f32, sgl_gather_rows_bf16_f32 and sgl_gather_hops_bf16_f32 with the source far, the destination far, and both:
    bit-equal to numpy fancy indexing (exact widening for bfloat16)"""
    n, H = N, 4
    idx_h = index_list(n)
    idx = torch.from_numpy(idx_h).to(cuda)
    perm_h = np.random.default_rng(3).permutation(n).astype(np.int64)
    perm = torch.from_numpy(perm_h).to(cuda)
    src_rows = torch.from_numpy(np.where(idx_h < 0, idx_h + n, idx_h)).to(cuda)          # the scatter takes plain row numbers
    with family(far, "gathers and scatter", n, cuda) as fam:
        for d in WIDTHS:
            hosts = hops_host(n, d, H, seed=1)
            hosts16 = [rne(h) for h in hosts]
            dp = dev.round_up(d, 4)
            for where in ("fn", "nf", "ff"):
                ctx = (d, where)

                def plain(bs, bd):
                    x, o = bs.inp(hosts[0]), bd.out(n, d)
                    call("sgl_gather_rows_f32", P(x), ld(x), n, P(idx), n, P(o), ld(o), d)
                    return {"out": o}
                assert np.array_equal(fam.both(plain, where)["out"].numpy(), hosts[0][idx_h]), ctx

                def padded(bs, bd):
                    x, o, o2 = bs.inp(hosts[1]), bd.out(n, d), bd.out(n, d)
                    call("sgl_gather_rows_padded_f32", P(x), ld(x), n, P(idx), n, P(o), ld(o), d, dp - d)
                    dev.gather_rows(x, idx, out=o2)
                    return {"abi": o, "wrapper": o2}
                got = fam.both(padded, where)
                assert np.array_equal(got["abi"].numpy(), hosts[1][idx_h]) and np.array_equal(got["wrapper"].numpy(), hosts[1][idx_h]), ctx

                def many(bs, bd):
                    xs, outs = [bs.inp(h) for h in hosts], [bd.out(n, d) for _ in hosts]
                    ptrs, lds = _lib.hop_arrays(xs)
                    optrs, olds = _lib.hop_arrays(outs)
                    call("sgl_gather_hops_padded_f32", H, ptrs, lds, n, P(idx), n, optrs, olds, d, dp - d)
                    return {f"out{h}": o for h, o in enumerate(outs)}
                got = fam.both(many, where)
                assert all(np.array_equal(got[f"out{h}"].numpy(), hosts[h][idx_h]) for h in range(H)), ctx

                def scatter(bs, bd):
                    x, o = bs.inp(hosts[2]), bd.out(n, d)
                    dev.scatter_rows(x, src_rows, perm, o)
                    return {"out": o}
                want = np.empty_like(hosts[2])
                want[perm_h] = hosts[2][idx_h]
                assert np.array_equal(fam.both(scatter, where)["out"].numpy(), want), ctx

                def bf16_rows(bs, bd):
                    x, o, o2 = bs.inp(hosts16[0]), bd.out(n, d), bd.out(n, d)
                    call("sgl_gather_rows_bf16_f32", P(x), ld(x), n, P(idx), n, P(o), ld(o), d, 0)
                    dev.gather_rows(x, idx, out=o2)
                    return {"abi": o, "wrapper": o2}
                got = fam.both(bf16_rows, where)
                want = hosts16[0].float().numpy()[idx_h]
                assert np.array_equal(got["abi"].numpy(), want) and np.array_equal(got["wrapper"].numpy(), want), ctx

                def bf16_many(bs, bd):
                    xs, outs = [bs.inp(h) for h in hosts16], [bd.out(n, d) for _ in hosts16]
                    ptrs, lds = _lib.hop_arrays(xs)
                    optrs, olds = _lib.hop_arrays(outs)
                    call("sgl_gather_hops_bf16_f32", H, ptrs, lds, n, P(idx), n, optrs, olds, d, 0)
                    return {f"out{h}": o for h, o in enumerate(outs)}
                got = fam.both(bf16_many, where)
                assert all(np.array_equal(got[f"out{h}"].numpy(), hosts16[h].float().numpy()[idx_h]) for h in range(H)), ctx


# ---- float32 aggregators --------------------------------------------------------------------------------------------------------------
def hop_weights(H):
    return (np.float32(0.75) ** np.arange(H, dtype=np.float32) * np.where(np.arange(H) % 3 == 2, -1, 1)).astype(np.float32)


def test_reduce_and_weighted_sums_f32(cuda, far):
    """sgl_hop_reduce_f32 with every op: sum / mean / max / min bit-equal to the oracle (test_simple_aggregators_bit_exact,
    test_aggregators_fuzz_random_shapes), the weighted sum under the fuzz test's parity bar; sgl_hop_wsum2d_f32 under the same bar
    with a far W; its backward: dW against float64 through truth_report (the statement of test_gpu_agg_variants.py), dX = W dOut,
    one IEEE product per element, bit-equal; sgl_hop_wsum1d_bwd_f32 and sgl_hop_rowdot_f32 under the fuzz test's bars"""
    n = N
    with family(far, "reduce / wsum2d (+bwd) / wsum1d_bwd / rowdot", n, cuda) as fam:
        for d in WIDTHS:
            for H in HOPS:
                hosts = hops_host(n, d, H)
                w1 = hop_weights(H)
                w1d = torch.from_numpy(w1).to(cuda)
                ctx = (d, H)
                for kind, op in OPS.items():
                    def reduce(b):
                        xs, o = [b.inp(h) for h in hosts], b.out(n, d)
                        ptrs, lds = _lib.hop_arrays(xs)
                        call("sgl_hop_reduce_f32", op, H, ptrs, lds, P(w1d) if kind == "wsum" else None, P(o), ld(o), n, d)
                        return {"out": o}
                    y = fam.both(reduce)["out"].numpy()
                    if kind == "wsum":
                        assert oracle.parity_ok(y, oracle.one_dim_weighted_add(hosts, w1), 1e-5, rowwise=False), (ctx, kind)
                    else:
                        want = {"sum": oracle.agg_sum, "mean": oracle.agg_mean, "max": oracle.agg_max, "min": oracle.agg_min}[kind](hosts, 0, H)
                        assert np.array_equal(y, want), (ctx, kind)
                        assert same_bits32(y, reduce_statement(kind, hosts, w1)), (ctx, kind)

                w2 = oracle.softmax32(hash_matrix(n, H, seed=d + H), 1)
                g = hash_matrix(n, d, seed=5 * d + 2)

                def wsum2d(b):
                    xs, w, o = [b.inp(h) for h in hosts], b.inp(w2), b.out(n, d)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_hop_wsum2d_f32", H, ptrs, lds, P(w), ld(w), P(o), ld(o), n, d)
                    return {"out": o}
                assert oracle.parity_ok(fam.both(wsum2d)["out"].numpy(), oracle.two_dim_weighted_add(hosts, w2), 1e-5, rowwise=False), ctx

                def wsum2d_bwd(b):
                    xs, w, go, dw = [b.inp(h) for h in hosts], b.inp(w2), b.inp(g), b.out(n, H)
                    dxs = [b.out(n, d) for _ in hosts]
                    ptrs, lds = _lib.hop_arrays(xs)
                    dptrs, dlds = _lib.hop_arrays(dxs)
                    call("sgl_hop_wsum2d_bwd_f32", H, ptrs, lds, P(w), ld(w), P(go), ld(go), P(dw), ld(dw), dptrs, dlds, n, d)
                    return dict({"dW": dw}, **{f"dX{h}": t for h, t in enumerate(dxs)})
                got = fam.both(wsum2d_bwd)
                g64 = t64(g)
                assert truth_ok(got["dW"].numpy(), torch.stack([(t32(g) * t32(x)).sum(1) for x in hosts], 1),
                                torch.stack([(g64 * t64(x)).sum(1) for x in hosts], 1),
                                cond=torch.stack([(g64.abs() * t64(x).abs()).sum(1) for x in hosts], 1)), ctx
                assert all(np.array_equal(got[f"dX{h}"].numpy(), w2[:, h:h + 1] * g) for h in range(H)), ctx

                scratch = torch.empty(int(_lib.lib().sgl_hop_wsum1d_bwd_scratch(H)), dtype=torch.float32, device=cuda)

                def wsum1d_bwd(b):
                    xs, go = [b.inp(h) for h in hosts], b.inp(g)
                    dw = torch.full((H,), NAN, dtype=torch.float32, device=cuda)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_hop_wsum1d_bwd_f32", H, ptrs, lds, P(go), ld(go), P(dw), P(scratch), n, d)
                    return {"dw": dw}
                ref1 = np.array([(g.astype(np.float64) * x).sum() for x in hosts])
                assert np.allclose(fam.both(wsum1d_bwd)["dw"].numpy(), ref1, rtol=2e-4, atol=2e-4 * max(1.0, np.abs(ref1).max())), ctx

                v = vector(d, 7 * d + 1, 0.3)
                vp = dev._padded_vec(torch.from_numpy(v), d, cuda)

                def rowdot(b):
                    xs, o = [b.inp(h) for h in hosts], b.out(n, H)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_hop_rowdot_f32", H, ptrs, lds, P(vp), P(o), ld(o), n, d)
                    return {"out": o}
                ref = np.stack([x.astype(np.float64) @ v for x in hosts], 1)
                assert np.allclose(fam.both(rowdot)["out"].numpy(), ref, rtol=2e-4, atol=2e-4 * max(1.0, np.abs(ref).max())), ctx


def test_rowdot2_lincomb_select_bwd_f32(cuda, far):
    """sgl_hop_rowdot2_f32 (far P and far U at a row step; statement and bar of test_gpu_agg_variants.rowdot2_case), sgl_hop_lincomb_f32 (near weights: its
    ldw is capped below 2^31; one fma chain per output in j order, under the parity bar of the weighted sums) and
    sgl_hop_select_bwd_f32 against torch's autograd of stack(...).max / min, bit-equal (test_round5_kernels_fuzz_random_shapes)"""
    n = N
    with family(far, "rowdot2 / lincomb / select_bwd", n, cuda) as fam:
        for d in WIDTHS:
            for H in HOPS:
                hosts = hops_host(n, d, H)
                ctx = (d, H)
                v = vector(d, 13 * d + 5, 0.3)
                u = np.ascontiguousarray(hash_matrix(H, d, seed=17 * d + H) * np.float32(0.3))
                mask = (0xB6DB & ((1 << H) - 1)) | (1 << (H - 1))
                h0, h1 = 1, H
                vp = dev._padded_vec(torch.from_numpy(v), d, cuda)

                def rowdot2(b):
                    xs, p = [b.inp(h) for h in hosts], b.out(n, h1 - h0)
                    up = b.inp(u, step=(n - 1) // (H - 1))                      # U [H, ldu]: far too, every (n - 1) // (H - 1)-th row
                    a = torch.full((n,), NAN, dtype=torch.float32, device=cuda)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_hop_rowdot2_f32", H, ptrs, lds, P(up), ld(up), mask, P(vp), h0, h1, P(p), ld(p), P(a), n, d)
                    return {"P": p, "A": a}
                got = fam.both(rowdot2)
                ref_hops = [j for j in range(H) if (mask >> j) & 1]
                for what, res, terms in (("P", got["P"], [[(hosts[h], v)] for h in range(h0, h1)]),
                                         ("A", got["A"][:, None], [[(hosts[j], u[j]) for j in ref_hops]])):
                    truth = torch.stack([sum(t64(x) @ t64(y_) for x, y_ in c) for c in terms], 1)
                    ref32 = torch.stack([sum(t32(x) @ t32(y_) for x, y_ in c) for c in terms], 1)
                    cond = torch.stack([sum(t64(x).abs() @ t64(y_).abs() for x, y_ in c) for c in terms], 1)
                    assert truth_ok(res.numpy(), ref32, truth, cond=cond), (ctx, what)

                n_out = 3
                wl = np.ascontiguousarray(hash_matrix(n_out, H, seed=d + 3 * H))
                wl[1, 0] = 0.0                                                   # a skipped hop
                wld = torch.from_numpy(wl).to(cuda)

                def lincomb(b):
                    xs, outs = [b.inp(h) for h in hosts], [b.out(n, d) for _ in range(n_out)]
                    ptrs, lds = _lib.hop_arrays(xs)
                    optrs, olds = _lib.hop_arrays(outs)
                    call("sgl_hop_lincomb_f32", H, ptrs, lds, n_out, optrs, olds, P(wld), H, n, d)
                    return {f"out{k}": o for k, o in enumerate(outs)}
                got = fam.both(lincomb)
                want = np.einsum("kj,jnd->knd", wl.astype(np.float64), np.stack(hosts).astype(np.float64))
                scale = np.einsum("kj,jnd->knd", np.abs(wl).astype(np.float64), np.abs(np.stack(hosts)).astype(np.float64))
                for k in range(n_out):
                    assert np.abs(got[f"out{k}"].numpy() - want[k]).max() <= 1e-6 * max(scale[k].max(), 1e-30), (ctx, k)

                base = [h.copy() for h in hosts[:min(H, 9)]]
                base[2][0] = base[0][0]                                          # ties
                base[1][3, 0] = np.nan
                Hs = len(base)
                g = hash_matrix(n, d, seed=5 * d + 3)
                for op, name in ((_lib.SGL_REDUCE_MAX, "max"), (_lib.SGL_REDUCE_MIN, "min")):
                    def select(b):
                        xs, go, dxs = [b.inp(h) for h in base], b.inp(g), [b.out(n, d) for _ in base]
                        ptrs, lds = _lib.hop_arrays(xs)
                        dptrs, dlds = _lib.hop_arrays(dxs)
                        call("sgl_hop_select_bwd_f32", op, Hs, ptrs, lds, P(go), ld(go), dptrs, dlds, n, d)
                        return {f"dX{h}": t for h, t in enumerate(dxs)}
                    got = fam.both(select)
                    leaves = [torch.from_numpy(x.copy()).to(cuda).requires_grad_(True) for x in base]
                    getattr(torch.stack(leaves, 0), name)(0)[0].backward(torch.from_numpy(g).to(cuda))
                    assert all(torch.equal(got[f"dX{h}"], leaves[h].grad.cpu()) for h in range(Hs)), (ctx, name)


def test_concat_and_nafs_f32(cuda, far):
    """sgl_hop_concat_f32 / _padded (bit-equal to numpy's hstack), sgl_nafs_f32 / _padded with a far W and sgl_nafs_prefix_f32
    (the oracle under the bars of test_gpu_agg_variants.nafs_case / prefix_case)"""
    n = N
    with family(far, "concat / nafs / nafs_prefix", n, cuda) as fam:
        for d in WIDTHS:
            for H in HOPS:
                hosts = hops_host(n, d, H)
                ctx = (d, H)
                width = H * d
                pad = (-width) % 4 + 4

                def concat(b):
                    xs, o, o2 = [b.inp(h) for h in hosts], b.out(n, width), b.out(n, width + pad)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_hop_concat_f32", H, ptrs, lds, P(o), ld(o), n, d)
                    call("sgl_hop_concat_padded_f32", H, ptrs, lds, P(o2), ld(o2), pad, n, d)
                    return {"plain": o, "padded": o2}
                got = fam.both(concat)
                assert np.array_equal(got["plain"].numpy(), np.hstack(hosts)), ctx
                assert np.array_equal(got["padded"].numpy()[:, :width], np.hstack(hosts)) and not got["padded"].numpy()[:, width:].any(), ctx

                dpad = dev.round_up(d, 4) - d + 4

                def nafs(b):
                    xs = [b.inp(h) for h in hosts]
                    o, w, o2, w2 = b.out(n, d), b.out(n, H), b.out(n, d + dpad), b.out(n, H)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_nafs_f32", H, ptrs, lds, P(o), ld(o), P(w), ld(w), n, d)
                    call("sgl_nafs_padded_f32", H, ptrs, lds, P(o2), ld(o2), dpad, P(w2), ld(w2), n, d)
                    return {"out": o, "W": w, "out_padded": o2, "W_padded": w2}
                got = fam.both(nafs)
                y, w = got["out"].numpy(), got["W"].numpy()
                assert np.isfinite(y).all() and np.isfinite(w).all(), ctx
                assert np.allclose(w, oracle.nafs_weights(hosts), rtol=5e-5, atol=5e-6), ctx
                assert oracle.parity_ok(y, oracle.agg_over_smooth_distance(hosts), 2e-5, rowwise=False), ctx
                assert np.array_equal(got["out_padded"].numpy()[:, :d], y) and not got["out_padded"].numpy()[:, d:].any(), ctx
                assert np.array_equal(got["W_padded"].numpy(), w), ctx

                emit = sorted({0, H // 2, H - 1})
                emask = sum(1 << h for h in emit)

                def prefix(b):
                    xs, outs = [b.inp(h) for h in hosts], [b.out(n, d) for _ in emit]
                    ptrs, lds = _lib.hop_arrays(xs)
                    optrs, olds = _lib.hop_arrays(outs)
                    call("sgl_nafs_prefix_f32", H, ptrs, lds, emask, optrs, olds, 0, 0, 1.0, n, d)
                    return {f"prefix{h}": o for h, o in zip(emit, outs)}
                got = fam.both(prefix)
                for h in emit:
                    p = got[f"prefix{h}"].numpy()
                    assert np.isfinite(p).all() and oracle.parity_ok(p, oracle.agg_over_smooth_distance(hosts[:h + 1]), 2e-5, rowwise=False), (ctx, h)


def test_concat_padded_writes_its_pad_columns_in_every_branch(cuda):
    """sgl_hop_concat_padded_f32 writes the declared pad columns as zeros whichever kernel its launcher picks.  The far test above
    found them untouched where d is a multiple of 4 (the 16-byte copy kernel wrote the row's width only, and so did the float-by-float
    one behind dense unaligned hops or d < 4): ordinary buffers, no table needed.  One case per branch of the launcher, in its
    order: hop_concat_kernel<4> (d = 104, 8), hop_concat_rows_kernel (147, 65: rows of 256 .. 4096 floats), hop_concat_lds_kernel
    (1029: a row of 4116 floats, beyond the whole-row kernel), hop_concat_any_kernel (7: a row under 256 floats),
    hop_concat_kernel<1> (dense hops of 6 columns, whose rows are not 16-byte vectors; d = 3)"""
    n, H = 77, 4
    near = Near(cuda)
    for d, dense in ((104, False), (8, False), (147, False), (65, False), (1029, False), (7, False), (6, True), (3, False)):
        hosts = hops_host(n, d, H, seed=3)
        xs = [torch.from_numpy(h).to(cuda) if dense else near.inp(h) for h in hosts]
        width = H * d
        pad = (-width) % 4 + 4
        o = near.out(n, width + pad)                                             # holds the NaN fill
        ptrs, lds = _lib.hop_arrays(xs)
        call("sgl_hop_concat_padded_f32", H, ptrs, lds, P(o), ld(o), pad, n, d)
        got = o.cpu().numpy()
        assert np.array_equal(got[:, :width], np.hstack(hosts)) and not got[:, width:].view(np.uint32).any(), (d, dense)


def recursive_bwd_reference(a, c, bias, g, dt):
    """(dA, dC, dB per row) of W = recursive_weights(A, C, b) under the upstream gradient G, by torch autograd in dtype dt"""
    a_, c_ = torch.from_numpy(a).to(dt).requires_grad_(True), torch.from_numpy(c).to(dt).requires_grad_(True)
    b_ = torch.full((a.shape[0],), bias, dtype=torch.float32).to(dt).requires_grad_(True)
    w = dev.recursive_weights(a_, c_, b_)
    (w * torch.from_numpy(g).to(dt)).sum().backward()
    return a_.grad, c_.grad, b_.grad


def test_gate_and_recursive_f32(cuda, far):
    """sgl_hop_gate_f32 / _padded and sgl_hop_recursive_f32 with far W / G / A / C matrices, against their float64 statements
    through truth_report (test_gpu_agg_variants.gate_case / recursive_case); sgl_hop_recursive_bwd_f32 with every [n, H] matrix
    far against the autograd of the same recursion in float64, through truth_report"""
    n = N
    with family(far, "gate / recursive (+bwd)", n, cuda) as fam:
        for d in WIDTHS:
            for H in HOPS:
                hosts = hops_host(n, d, H)
                ctx = (d, H)
                v = vector(d, 7 * d + 1, 0.3)
                vp = dev._padded_vec(torch.from_numpy(v), d, cuda, tail=torch.tensor([BIAS]))
                dpad = dev.round_up(d, 4) - d + 4

                def gate(b):
                    xs = [b.inp(h) for h in hosts]
                    o, w, g_, o2, w2, g2 = b.out(n, d), b.out(n, H), b.out(n, H), b.out(n, d + dpad), b.out(n, H), b.out(n, H)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_hop_gate_f32", H, ptrs, lds, P(vp), BIAS, P(o), ld(o), P(w), ld(w), P(g_), ld(g_), n, d)
                    call("sgl_hop_gate_padded_f32", H, ptrs, lds, P(vp), NAN, P(o2), ld(o2), dpad, P(w2), ld(w2), P(g2), ld(g2), n, d)
                    return {"out": o, "W": w, "G": g_, "out_padded": o2, "W_padded": w2, "G_padded": g2}
                got = fam.both(gate)
                y64, w64, g64 = gate_reference(hosts, v, torch.float64)
                y32, w32, g32 = gate_reference(hosts, v, torch.float32)
                assert truth_ok(got["out"].numpy(), y32, y64) and truth_ok(got["W"].numpy(), w32, w64) and truth_ok(got["G"].numpy(), g32, g64), ctx
                assert np.array_equal(got["out_padded"].numpy()[:, :d], got["out"].numpy()) and not got["out_padded"].numpy()[:, d:].any(), ctx
                assert torch.equal(got["W_padded"], got["W"]) and torch.equal(got["G_padded"], got["G"]), ctx

                wt = vector(2 * d, 11 * d + 3, 0.5 / d ** 0.5)
                dp = dev.round_up(d, 4)
                rv = torch.zeros(2 * dp + 4, dtype=torch.float32)
                rv[:d], rv[dp:dp + d], rv[2 * dp] = torch.from_numpy(wt[:d]), torch.from_numpy(wt[d:]), BIAS
                rv = rv.to(cuda)

                def recursive(b):
                    xs = [b.inp(h) for h in hosts]
                    o, w, a, c = b.out(n, d), b.out(n, H), b.out(n, H), b.out(n, H)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_hop_recursive_f32", H, ptrs, lds, P(rv), NAN, P(o), ld(o), 0, P(w), ld(w), P(a), ld(a), P(c), ld(c), n, d)
                    return {"out": o, "W": w, "A": a, "C": c}
                got = fam.both(recursive)
                ref = {}
                for dt in (torch.float64, torch.float32):
                    ff = [torch.from_numpy(x).to(dt) for x in hosts]
                    wv = torch.from_numpy(wt).to(dt)
                    y, wr = recursive_step_by_step(ff, wv, torch.tensor([BIAS], dtype=torch.float32).to(dt))
                    ref[dt] = (y, wr, torch.stack([f @ wv[:d] for f in ff], 1), torch.stack([f @ wv[d:] for f in ff], 1))
                conds = [torch.stack([torch.from_numpy(np.abs(x)).double() @ torch.from_numpy(np.abs(part)).double() for x in hosts], 1)
                         for part in (wt[:d], wt[d:])]
                r64, r32 = ref[torch.float64], ref[torch.float32]
                assert truth_ok(got["out"].numpy(), r32[0], r64[0]) and truth_ok(got["W"].numpy(), r32[1], r64[1]), ctx
                assert truth_ok(got["A"].numpy(), r32[2], r64[2], cond=conds[0]) and truth_ok(got["C"].numpy(), r32[3], r64[3], cond=conds[1]), ctx

                a_h, c_h = got["A"].numpy().copy(), got["C"].numpy().copy()
                gw = np.ascontiguousarray(hash_matrix(n, H, seed=3 * d + H))

                def recursive_bwd(b):
                    a, c, g_ = b.inp(a_h), b.inp(c_h), b.inp(gw)
                    da, dc = b.out(n, H), b.out(n, H)
                    db = torch.full((n,), NAN, dtype=torch.float32, device=cuda)
                    call("sgl_hop_recursive_bwd_f32", H, P(a), ld(a), P(c), ld(c), BIAS, None, P(g_), ld(g_), P(da), ld(da), P(dc), ld(dc),
                         P(db), n)
                    return {"dA": da, "dC": dc, "dB": db}
                got = fam.both(recursive_bwd)
                t64_, t32_ = (recursive_bwd_reference(a_h, c_h, BIAS, gw, dt) for dt in (torch.float64, torch.float32))
                for k, what in enumerate(("dA", "dC", "dB")):
                    assert truth_ok(got[what].numpy(), t32_[k].numpy(), t64_[k].numpy()), (ctx, what)


def test_colsum_and_signature_f32(cuda, far):
    """sgl_hop_colsum_f32 (far hops, far W, far [H, ldo] output) against float64 under the bar of
    test_hop_colsum_is_the_weight_gradient_of_the_row_dots; sgl_col_signature_f32 bit-equal to its definition"""
    n = N
    with family(far, "colsum / col_signature", n, cuda) as fam:
        for d in WIDTHS:
            for H in HOPS:
                hosts = hops_host(n, d, H)
                ctx = (d, H)
                w = np.ascontiguousarray(hash_matrix(n, H, seed=9 * d + H))
                scratch = torch.empty(int(_lib.lib().sgl_hop_colsum_scratch(H, n, d)), dtype=torch.float32, device=cuda)

                def colsum(b):
                    xs, wd = [b.inp(h) for h in hosts], b.inp(w)
                    o, o_shared = b.out(H, d, step=(n - 1) // (H - 1)), b.out(H, d, step=(n - 1) // (H - 1))
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_hop_colsum_f32", H, ptrs, lds, P(wd), ld(wd), 1, P(o), ld(o), P(scratch), n, d)
                    call("sgl_hop_colsum_f32", H, ptrs, lds, P(wd), ld(wd), 0, P(o_shared), ld(o_shared), P(scratch), n, d)
                    return {"out": o, "shared": o_shared}
                got = fam.both(colsum)
                feats, wt = [t64(x) for x in hosts], t64(w)
                for key, col in (("out", lambda h: wt[:, h]), ("shared", lambda h: wt[:, 0])):
                    want = torch.stack([f.t() @ col(h) for h, f in enumerate(feats)])
                    mag = torch.stack([f.abs().t() @ col(h).abs() for h, f in enumerate(feats)]).clamp_min(1e-30)
                    assert float(((got[key].double() - want).abs() / mag).max()) <= 2e-6, (ctx, key)

            x = hosts[0]
            dw = dev.round_up(d, 4)

            def signature(b):
                xd = b.inp(x)
                sig = dev.column_signature(xd)
                assert sig is not None and sig.numel() == dw
                full = torch.as_strided(xd, (n, dw), (xd.stride(0), 1), xd.storage_offset())     # the columns the kernel reads
                return {"sig": sig, "read": full}
            got = fam.both(signature)
            with np.errstate(over="ignore"):
                want = sig_mix(got["read"].numpy().view(np.uint32), np.arange(n, dtype=np.uint64)[:, None]).sum(axis=0, dtype=np.uint64)
            assert np.array_equal(got["sig"].numpy().view(np.uint64), want), d


# ---- bfloat16 aggregators -------------------------------------------------------------------------------------------------------------
def test_aggregators_bf16(cuda, far):
    """sgl_hop_reduce_bf16_f32, sgl_hop_concat_bf16, sgl_hop_concat_bf16_f32 and sgl_nafs_bf16_f32 over far bfloat16 hops: bit-equal
    to "widen, then the float32 entry on near buffers" (test_gpu_bf16_agg.py), and against the float32 statement / the oracle of the
    float32 entry"""
    n = N
    with family(far, "bf16 reduce / concat / nafs", n, cuda) as fam:
        for d in WIDTHS:
            for H in HOPS:
                hosts16 = [rne(h) for h in hops_host(n, d, H, seed=2)]
                wide = [h.float().numpy() for h in hosts16]
                widened = dev.widen_hops([h.to(cuda) for h in hosts16])                  # row-padded float32 copies, near
                ctx = (d, H)
                w1 = hop_weights(H)
                w1d = torch.from_numpy(w1).to(cuda)
                for kind, op in OPS.items():
                    def reduce(b):
                        xs, o = [b.inp(h) for h in hosts16], b.out(n, d)
                        ptrs, lds = _lib.hop_arrays(xs)
                        call("sgl_hop_reduce_bf16_f32", op, H, ptrs, lds, P(w1d) if kind == "wsum" else None, P(o), ld(o), 0, n, d)
                        return {"out": o}
                    y = fam.both(reduce)["out"].numpy()
                    assert same_bits32(y, reduce_statement(kind, wide, w1)), (ctx, kind)
                    assert same_bits32(y, dev.hop_reduce(op, widened, w1d if kind == "wsum" else None).cpu().numpy()), (ctx, kind)
                    if kind == "wsum":                                           # ... and the references of the float32 entry
                        assert oracle.parity_ok(y, oracle.one_dim_weighted_add(wide, w1), 1e-5, rowwise=False), (ctx, kind)
                    else:
                        want = {"sum": oracle.agg_sum, "mean": oracle.agg_mean, "max": oracle.agg_max, "min": oracle.agg_min}[kind](wide, 0, H)
                        assert np.array_equal(y, want), (ctx, kind)

                def concat(b):
                    xs, o16, o32 = [b.inp(h) for h in hosts16], b.out(n, H * d, torch.bfloat16), b.out(n, H * d)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_hop_concat_bf16", H, ptrs, lds, P(o16), ld(o16), 0, n, d)
                    call("sgl_hop_concat_bf16_f32", H, ptrs, lds, P(o32), ld(o32), 0, n, d)
                    return {"bf16": o16, "f32": o32}
                got = fam.both(concat)
                assert np.array_equal(bits16(got["bf16"]), bits16(torch.cat(hosts16, dim=1))), ctx
                assert np.array_equal(got["f32"].numpy().view(np.uint32), np.hstack(wide).view(np.uint32)), ctx
                assert torch.equal(got["f32"], dev.hop_concat(widened).cpu()), ctx

                def nafs(b):
                    xs, o, w = [b.inp(h) for h in hosts16], b.out(n, d), b.out(n, H)
                    ptrs, lds = _lib.hop_arrays(xs)
                    call("sgl_nafs_bf16_f32", H, ptrs, lds, P(o), ld(o), 0, P(w), ld(w), n, d)
                    return {"out": o, "W": w}
                got = fam.both(nafs)
                y32, w32 = dev.nafs_aggregate(widened, return_weights=True)
                assert torch.equal(got["out"], y32.cpu()) and torch.equal(got["W"], w32.cpu()), ctx
                assert np.allclose(got["W"].numpy(), oracle.nafs_weights(wide), rtol=5e-5, atol=5e-6), ctx
                assert oracle.parity_ok(got["out"].numpy(), oracle.agg_over_smooth_distance(wide), 2e-5, rowwise=False), ctx


# ---- edge scores and k-means ----------------------------------------------------------------------------------------------------------
def test_edge_dot(cuda, far):
    """sgl_edge_dot_f32, same-matrix and two-matrix forms, over far matrices (C ABI and dev.edge_dot(out=)); the edge list of
    edge_scores_common joins first and last rows; the output is an ordinary vector.  The float64 row dot through truth_report with
    cond, as test_gpu_edge_scores.py compares it"""
    n = esc.N_ROWS
    edges = torch.from_numpy(esc.EDGES).to(cuda)
    n_e = esc.N_EDGES
    with family(far, "edge_dot", n, cuda) as fam:
        for d in WIDTHS:
            for two in (False, True):
                a_h, b_h = esc.host_matrix(d), esc.host_matrix(d, 1)

                def dot(b):
                    a = b.inp(a_h)
                    bb = b.inp(b_h) if two else a
                    o = torch.full((n_e,), NAN, dtype=torch.float32, device=cuda)
                    o2 = torch.full((n_e,), NAN, dtype=torch.float32, device=cuda)
                    call("sgl_edge_dot_f32", P(a), ld(a), n, P(bb), ld(bb), n, P(edges), n_e, d, P(o))
                    dev.edge_dot(a, bb, edges, out=o2)
                    return {"abi": o, "wrapper": o2}
                got = fam.both(dot)
                ref32, truth, cond = esc.references(d, two)
                assert truth_ok(got["abi"].numpy(), ref32, truth, cond=cond), (d, two)
                assert torch.equal(got["abi"], got["wrapper"]), (d, two)


def test_kmeans_assign(cuda, far):
    """sgl_kmeans_assign_f32 with X far and the k = 64 centres far as every 16th row of the table (the pitch is computed for
    (k - 1) * 16 + 1 rows, so (k - 1) * ldc is beyond the threshold too); several LDS tiles are staged.  Labels and mindist against
    the float64 reference of kmeans_common.py under its derived bars"""
    n, k = kc.N_ROWS, 64
    s = (n - 1) // (k - 1)
    with family(far, "kmeans_assign", n, cuda, pitch_rows=(k - 1) * s + 1) as fam:
        for d in WIDTHS + (600,):                                            # k * d = 38 400 floats at d = 600: three 64 KiB tiles
            x_h, c_h = kc.host_x(d), kc.host_centres(d, k)

            def assign(b):
                x, c = b.inp(x_h), b.inp(c_h, step=s)
                labels = torch.full((n,), -7, dtype=torch.int64, device=cuda)
                mind = torch.full((n,), NAN, dtype=torch.float32, device=cuda)
                call("sgl_kmeans_assign_f32", P(x), ld(x), n, d, P(c), ld(c), k, P(labels), P(mind))
                l2, m2 = dev.kmeans_assign(x, c)
                return {"labels": labels, "mindist": mind, "labels_wrapper": l2, "mindist_wrapper": m2}
            got = fam.both(assign)
            assert fam.lay.ld * s * (k - 1) > far.threshold
            labels, d1, near = kc.reference(d, k)
            assert near.mean() <= kc.MAX_LEFT_OUT, d
            keep = ~near
            assert np.array_equal(got["labels"].numpy()[keep], labels[keep]), d
            assert np.all(np.abs(got["mindist"].numpy().astype(np.float64) - d1) <= kc.dist_tol(d) * d1), d
            assert torch.equal(got["labels"], got["labels_wrapper"]) and torch.equal(got["mindist"], got["mindist_wrapper"]), d


def mix_torch(bits, r):
    """sig_mix in torch int64 arithmetic (wrapping; logical shifts spelled out): bits int32 [m, d], r int64 [m, 1]"""
    def shr(x, k):
        return (x >> k) & ((1 << (64 - k)) - 1)

    def c(v):                                        # a uint64 constant as the int64 with the same bits
        return v - (1 << 64) if v >= (1 << 63) else v
    h = ((bits.to(torch.int64) & 0xFFFFFFFF) ^ (r * c(0x9E3779B97F4A7C15))) * c(0xBF58476D1CE4E5B9)
    h = h ^ shr(h, 31)
    h = h * c(0x94D049BB133111EB)
    return h ^ shr(h, 29)

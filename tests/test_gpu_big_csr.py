"""Every entry point that forms a position into a CSR's col / val, at positions beyond 2^31 (tier B) and 2^32 (tier A): run with
`-m gpu`.  The sparse counterpart of test_gpu_far_offsets.py, by the same method: ONE large structure generated on the device by
formula (big_csr_common.py), references evaluated only where they are cheap -- on about 64 `near` rows (all entries below 2^30) and
more than 256 `far` rows (every row straddling a boundary, and rows of every class that start beyond it) -- and a CPU file
(test_big_csr_cpu.py) that proves the references right at a small size and the cases not blind.  The bar of every comparison is the
bar of the entry point's own small test: bits where that is bits.

The tests are written in the order in which they share a matrix: the directed tier-B matrix, the symmetric one, the directed tier-A
one.  Exactly one is alive at a time (matrix() frees the others); its build time is printed, and so is the peak of the device memory
in use during every case.  A tier that does not fit the free
device memory skips and says how much there was -- on an idle MI355X (288 GB) nothing skips."""
import ctypes
import gc
import threading
import time
from ctypes import c_int64

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import big_csr_common as big
import csr_select_common
import edge_split_common
import spmm_order_common as order
from oracle import ref_ops as oracle
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.io import DeviceAdjacency
from sgl_amd._lib import ptr

pytestmark = pytest.mark.gpu

HOLD = {}
NAN32, NAN64 = float("nan"), float("nan")


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    yield torch.device("cuda", 0)
    release()


@pytest.fixture(autouse=True)
def peak_memory(request, cuda):
    """prints the peak of the device memory in use during the case (the library's own hipMalloc temporaries included, which torch's
    counters do not see): a thread samples the free memory of the device every few milliseconds"""
    _, total = torch.cuda.mem_get_info()
    low, stop = [total], threading.Event()

    def sample():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(cuda)[0])
            stop.wait(0.004)

    th = threading.Thread(target=sample, daemon=True)
    th.start()
    yield
    stop.set()
    th.join()
    print(f"[big csr] {request.node.name}: peak device memory in use {(total - low[0]) / big.GIB:.1f} GiB")


def release():
    HOLD.clear()
    gc.collect()
    torch.cuda.empty_cache()


def need(nbytes, what):
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes / big.GIB:.0f} GiB of free device memory: {free / big.GIB:.1f} of {total / big.GIB:.0f} GiB are free")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Matrix:
    """the generated matrix on the device, its sampled rows and their sub-matrix"""

    def __init__(self, cuda, kind, tier):
        self.g = g = big.instance(kind, tier)
        self.kind, self.tier, self.cuda = kind, tier, cuda
        self.bounds = big.boundaries(tier)
        t0 = time.perf_counter()
        self.rowptr, self.col, self.val = g.generate(cuda)
        torch.cuda.synchronize()
        self.build_seconds = time.perf_counter() - t0
        print(f"\n[big csr] {kind} tier {tier}: n = {g.n}, nnz = {g.nnz} = {'2^31' if tier == 'B' else '2^32'} + {g.nnz - self.bounds[-1]}, generated in {self.build_seconds:.2f} s")
        self.near, self.far = g.near_rows(), g.far_rows(self.bounds)
        self.rows = np.concatenate((self.near, self.far))
        self.rows_t = torch.from_numpy(self.rows).to(cuda)
        self.indptr, self.idx, self.vals, self.cols = g.sub_matrix(self.rows)
        self.cols_t = torch.from_numpy(self.cols).to(cuda)
        self.adj = DeviceAdjacency(self.rowptr, self.col, self.val, (g.n, g.n))
        self.perm = None
        self.norm = None

    def norm_references(self):
        """(row pointer of A_hat on the device and on the host, rows without a stored diagonal, sampled Laplacian rows, sampled PPR rows)
        for r = 0.5, alpha = 0.15, once per matrix"""
        if self.norm is None:
            want_ptr, n_new = normalised_rowptr(self)
            degs = {}
            self.norm = (want_ptr, want_ptr.cpu().numpy(), n_new, big.norm_rows_reference(self.g, self.rows, 0.5, None, degs),
                         big.norm_rows_reference(self.g, self.rows, 0.5, 0.15, degs))
        return self.norm

    def positions(self, rowptr, rows):
        """the positions of the rows `rows` of a CSR with the HOST row pointer `rowptr`, one after the other, as a device index"""
        p = np.concatenate([np.arange(rowptr[i], rowptr[i + 1], dtype=np.int64) for i in rows] + [np.zeros(0, np.int64)])
        return torch.from_numpy(p).to(self.cuda)

    def permuted(self):
        """(perm, rowptr, col, val) of sgl_csr_permute_rows under the reversal: the near rows go to the far end and back"""
        if self.perm is None:
            n, nnz = self.g.n, self.g.nnz
            perm = (n - 1 - torch.arange(n, dtype=torch.int64, device=self.cuda)).to(torch.int32)
            o_ptr = torch.full((n + 1,), -1, dtype=torch.int64, device=self.cuda)
            o_col = torch.full((nnz,), -1, dtype=torch.int32, device=self.cuda)
            o_val = torch.full((nnz,), NAN32, dtype=torch.float32, device=self.cuda)
            dev._call(self.cuda, "sgl_csr_permute_rows", ptr(self.rowptr), ptr(self.col), ptr(self.val), n, ptr(perm), ptr(o_ptr), ptr(o_col), ptr(o_val))
            self.perm = (perm, o_ptr, o_col, o_val)
        return self.perm


def matrix(cuda, kind, tier):
    key = (kind, tier)
    if HOLD.get("key") != key:
        release()
        need(big.TIERS[tier][1], f"tier {tier}")
        HOLD["key"], HOLD["m"] = key, Matrix(cuda, kind, tier)
    return HOLD["m"]


# ---- the fixture itself ------------------------------------------------------------------------------------------------------------
def test_generated_matrix_is_the_formula(cuda):
    check_generated(matrix(cuda, "directed", "B"))


def check_generated(m):
    g = m.g
    assert g.nnz > m.bounds[-1] + big.MARGIN and m.col.numel() == g.nnz
    pos = m.positions(g.rowptr, m.rows)
    assert int(pos.max()) > m.bounds[-1]
    want = [g.row(i) for i in m.rows]
    assert np.array_equal(m.col[pos].cpu().numpy(), np.concatenate([w[0] for w in want]).astype(np.int32))
    assert same_bits(m.val[pos].cpu().numpy(), np.concatenate([w[1] for w in want]))
    assert int(m.col.min()) >= 0 and int(m.col.max()) < g.n


# ---- SpMM --------------------------------------------------------------------------------------------------------------------------
VARIANTS = {"default": {}, "item64": dict(item_nnz=64), "cut": dict(long_row_nnz=big.SMALL_LONG_ROW_NNZ), "rowmap": {}}


def rows_of(m, t):
    return t[m.rows_t].cpu()


def sentinel(m, d, dtype=torch.float32):
    return torch.full((m.g.n, d), NAN32, dtype=dtype, device=m.cuda)


def written(t):
    return not bool(torch.isnan(t).any())


def group_ratio(dtype, d, x, y, avg):
    var = order.dispatch(dtype, d, x.stride(0), y.stride(0), x.data_ptr(), y.data_ptr(), False, avg)
    assert len(var) == 1
    return 64 // var[0][2][1]


def spmm_cases(m, fast, strict, d, lrn, full, mapped):
    g, cuda = m.g, m.cuda
    avg = g.nnz / g.n
    gen = torch.Generator(device=cuda).manual_seed(100 + d)
    x = torch.randn(g.n, d, generator=gen, device=cuda)
    xs = x[m.cols_t].cpu().numpy()
    sub = (m.indptr, m.idx, m.vals)
    want = oracle.oracle_spmm(*sub, xs)
    truth = sp.csr_matrix((m.vals.astype(np.float64), m.idx, m.indptr), shape=(len(m.rows), len(m.cols))) @ xs.astype(np.float64)
    # sgl_spmm_f32, strict order: the reference's chain, bit for bit
    y = sentinel(m, d)
    strict.spmm(x, out=y)
    assert written(y) and same_bits(rows_of(m, y).numpy(), want), ("strict", d)
    # fast order: the slot model bit for bit, and within the reference's own error of the float64 truth
    y = sentinel(m, d)
    fast.spmm(x, out=y)
    got = rows_of(m, y).numpy()
    assert written(y) and same_bits(got, oracle.oracle_spmm_slots(*sub, xs, group_ratio("f32", d, x, y, avg), lrn)), ("fast", d)
    rep = oracle.truth_report(got, want, truth)
    assert rep["ok"], ("fast", d, rep)
    # bfloat16 hops
    xb = x.to(torch.bfloat16)
    xbs = xb[m.cols_t].cpu()
    wantb = oracle.oracle_spmm_slots_bf16(*sub, xbs, 1, -1)
    yb = sentinel(m, d, torch.bfloat16)
    strict.spmm(xb, out=yb)
    assert written(yb) and torch.equal(rows_of(m, yb).view(torch.int16), wantb.view(torch.int16)), ("bf16 strict", d)
    yb2 = sentinel(m, d, torch.bfloat16)
    fast.spmm(xb, out=yb2)
    wantb2 = oracle.oracle_spmm_slots_bf16(*sub, xbs, group_ratio("bf16", d, xb, yb2, avg), lrn)
    assert written(yb2) and torch.equal(rows_of(m, yb2).view(torch.int16), wantb2.view(torch.int16)), ("bf16 fast", d)
    if not full:
        return
    # sgl_spmm_chain_f32, two hops: hop 2 against the reference product of the hop-1 rows the device produced
    y1, y2 = sentinel(m, d), sentinel(m, d)
    strict.spmm_chain(x, 2, outs=[y1, y2])
    assert written(y1) and written(y2) and same_bits(rows_of(m, y1).numpy(), want), ("chain 1", d)
    assert same_bits(rows_of(m, y2).numpy(), oracle.oracle_spmm(*sub, y1[m.cols_t].cpu().numpy())), ("chain 2", d)
    # sgl_spmm_multi_f32, one replica; a second replica is refused on a mapped handle (the replicas are addressed by storage row)
    y = sentinel(m, d)
    strict.spmm_multi(x, [y.data_ptr()], d)
    assert written(y) and same_bits(rows_of(m, y).numpy(), want), ("multi", d)
    if mapped:
        with pytest.raises(_lib.SglHipError):
            strict.spmm_multi(x, [y.data_ptr(), y.data_ptr()], d)
    # sgl_spmm_acc_f32: the running sum and the running maximum
    a0 = torch.randn(g.n, d, generator=gen, device=cuda)
    a0s = rows_of(m, a0).numpy()
    for mode, ref in (("sum", a0s + want), ("max", np.maximum(a0s, want))):
        acc, y = a0.clone(), sentinel(m, d)
        strict.spmm_acc(x, y, acc, mode=mode)
        assert written(y) and same_bits(rows_of(m, y).numpy(), want) and same_bits(rows_of(m, acc).numpy(), ref.astype(np.float32)), (mode, d)
    # sgl_spmm_axpb_clamp_f32: rounded product, rounded add, clamp
    y = sentinel(m, d)
    strict.spmm_axpb_clamp(x, 0.85, res=a0, lo=-0.5, hi=0.5, out=y)
    ref = np.clip((np.float32(0.85) * want).astype(np.float32) + a0s, np.float32(-0.5), np.float32(0.5)).astype(np.float32)
    assert written(y) and same_bits(rows_of(m, y).numpy(), ref), ("axpb", d)
    # sgl_spmm_chain_bf16 and sgl_spmm_acc_bf16
    y1, y2 = sentinel(m, d, torch.bfloat16), sentinel(m, d, torch.bfloat16)
    strict.spmm_chain(xb, 2, outs=[y1, y2])
    assert written(y1) and written(y2) and torch.equal(rows_of(m, y1).view(torch.int16), wantb.view(torch.int16)), ("bf16 chain 1", d)
    want2 = oracle.oracle_spmm_slots_bf16(*sub, y1[m.cols_t].cpu(), 1, -1)
    assert torch.equal(rows_of(m, y2).view(torch.int16), want2.view(torch.int16)), ("bf16 chain 2", d)
    acc, yb = a0.clone(), sentinel(m, d, torch.bfloat16)
    strict.spmm_acc(xb, yb, acc, mode="sum")
    assert torch.equal(rows_of(m, yb).view(torch.int16), wantb.view(torch.int16)), ("bf16 acc", d)
    assert same_bits(rows_of(m, acc).numpy(), (a0s + wantb.float().numpy()).astype(np.float32)), ("bf16 acc", d)


def spmm_family(cuda, tier, variant):
    m = matrix(cuda, "directed", tier)
    g = m.g
    kw = VARIANTS[variant]
    mapped = variant == "rowmap"
    arrays = m.permuted()[1:] if mapped else (m.rowptr, m.col, m.val)
    lrn = kw.get("long_row_nnz", order.default_long_row_nnz(g.nnz))
    t0 = time.perf_counter()
    fast = dev.DeviceCSR(*arrays, (g.n, g.n), **kw)
    strict = dev.DeviceCSR(*arrays, (g.n, g.n), strict=True, **kw)
    try:
        if mapped:
            fast.set_rowmap(m.permuted()[0])
            strict.set_rowmap(m.permuted()[0])
        cut = g.len > lrn
        info, sinfo = fast.info(), strict.info()
        assert (info["n_rows"], info["n_cols"], info["nnz"]) == (g.n, g.n, g.nnz) and lrn == (big.SMALL_LONG_ROW_NNZ if variant == "cut" else 2048)
        assert info["n_long_rows"] == cut.sum() > 0 and info["n_pieces"] == (-(-g.len[cut] // lrn)).sum()
        assert sinfo["n_long_rows"] == 0 and sinfo["n_pieces"] == 0 and sinfo["nnz"] == g.nnz
        for d in (1, 4, 8, 100):
            spmm_cases(m, fast, strict, d, lrn, tier == "B", mapped)
        torch.cuda.synchronize()
    finally:
        fast.close()
        strict.close()
    print(f"[big csr] SpMM family, tier {tier}, {variant}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_spmm_family(cuda, variant):
    spmm_family(cuda, "B", variant)


# ---- row permutation -----------------------------------------------------------------------------------------------------------------
def permute_rows_case(cuda, tier):
    m = matrix(cuda, "directed", tier)
    g = m.g
    t0 = time.perf_counter()
    perm, o_ptr, o_col, o_val = m.permuted()
    torch.cuda.synchronize()
    want_ptr = np.concatenate(([0], np.cumsum(g.len[::-1])))
    assert torch.equal(o_ptr, torch.from_numpy(want_ptr).to(cuda))
    assert int(o_col.min()) >= 0 and not bool(torch.isnan(o_val).any())                  # no sentinel is left
    ks = np.unique(np.concatenate((m.rows, g.n - 1 - m.rows)))                           # output rows near and far, fed from far and near
    pos = m.positions(want_ptr, ks)
    assert int(pos.max()) > m.bounds[-1]
    want = [g.row(g.n - 1 - k) for k in ks]
    assert np.array_equal(o_col[pos].cpu().numpy(), np.concatenate([w[0] for w in want]).astype(np.int32))
    assert same_bits(o_val[pos].cpu().numpy(), np.concatenate([w[1] for w in want]))
    only = torch.full((g.n + 1,), -1, dtype=torch.int64, device=cuda)                    # the row-pointer-only mode
    dev._call(cuda, "sgl_csr_permute_rows", ptr(m.rowptr), None, None, g.n, ptr(perm), ptr(only), None, None)
    assert torch.equal(only, o_ptr)
    print(f"[big csr] permute rows, tier {tier}: {time.perf_counter() - t0:.2f} s")


def test_permute_rows(cuda):
    permute_rows_case(cuda, "B")


# ---- lookup and sampling ---------------------------------------------------------------------------------------------------------------
def find_case(cuda, tier):
    m = matrix(cuda, "directed", tier)
    g = m.g
    t0 = time.perf_counter()
    q = []
    for i in m.rows.tolist():
        c = g.row(i)[0]
        for j in ([c[0], c[len(c) // 2], c[-1], c[0] - 1, c[-1] + 1, c[len(c) // 2] + 1] if len(c) else [i, 0]):
            if 0 <= j < g.n:
                q += [(i, j), (i - g.n, j - g.n)]                                          # and the same pair counted from the end
    q = np.asarray(q, dtype=np.int64)
    want = g.find(q[:, 0] % g.n, q[:, 1] % g.n)
    got = dev.csr_find(m.adj, torch.from_numpy(q).to(cuda)).cpu().numpy()
    assert np.array_equal(got, want) and want.max() > m.bounds[-1] and (want < 0).sum() > 100 and ((want >= 0) & (want < (1 << 30))).sum() > 100
    # a candidate window with a stored pair in a far row, found on the host from the formulas
    far0 = int(np.searchsorted(g.rowptr, m.bounds[-1], side="right") - 1)
    count, seed = 1 << 18, 77
    for w in range(64):
        pairs = edge_split_common.candidate_pairs(g.n, seed, w * count, count)
        pos = g.find(pairs[:, 0], pairs[:, 1])
        if (pos > m.bounds[-1]).any():
            break
    assert (pos > m.bounds[-1]).any() and (pairs[:, 0] > far0).sum() > 100
    free = (pairs[:, 0] != pairs[:, 1]) & (pos < 0)
    key = np.where(free, pairs.min(1) * g.n + pairs.max(1), -1)
    edges, got_key = dev.edge_candidates(m.adj, seed, w * count, count)
    assert np.array_equal(edges.cpu().numpy(), pairs) and np.array_equal(got_key.cpu().numpy(), key)
    print(f"[big csr] find and candidates, tier {tier}: {time.perf_counter() - t0:.2f} s")


def test_find_and_candidates(cuda):
    find_case(cuda, "B")


# ---- merge -----------------------------------------------------------------------------------------------------------------------------
def merge_case(cuda, tier, runs):
    m = matrix(cuda, "directed", tier)
    g = m.g
    t0 = time.perf_counter()
    ar = np.arange(g.n, dtype=np.int64)
    has_diag = g.find(ar, ar) >= 0
    extra = {}                                             # far and near rows get more than their self-loop: columns A stores, and new ones
    for i in np.concatenate((m.far[:48], m.near[:8])).tolist():
        c = g.row(i)[0]
        cand = ([c[0], c[-1], c[-1] + 1, c[0] + 1] if len(c) else [3, 4]) + [(i * 7 + 1) % g.n]
        extra[i] = np.setdiff1d(np.unique([j for j in cand if 0 <= j < g.n]), [i])
    bi = np.concatenate([ar] + [np.full(len(c), i) for i, c in extra.items()])
    bj = np.concatenate([ar] + list(extra.values()))
    bv = (1.0 + (big.hash_np(bj, bi) & 0xFFFF) / 65536.0).astype(np.float32)
    b = sp.csr_matrix((bv, (bi, bj)), shape=(g.n, g.n))
    b.sort_indices()
    assert b.has_canonical_format and b.nnz == len(bi)
    new = ~has_diag
    out_len = g.len + new
    for i, c in extra.items():
        out_len[i] += (g.find(np.full(len(c), i), c) < 0).sum()
    want_ptr = np.concatenate(([0], np.cumsum(out_len)))
    badj = DeviceAdjacency(torch.from_numpy(b.indptr.astype(np.int64)).to(cuda), torch.from_numpy(b.indices.astype(np.int32)).to(cuda),
                           torch.from_numpy(b.data).to(cuda), (g.n, g.n))
    want_ptr_t = torch.from_numpy(want_ptr).to(cuda)
    pos = m.positions(want_ptr, m.rows)
    for mode, lanes in runs:
        out, (pa, pb) = dev.csr_merge(m.adj, badj, mode=mode, lanes=lanes, positions=True)
        assert out.nnz == want_ptr[-1] > m.bounds[-1] and torch.equal(out.rowptr, want_ptr_t), (mode, lanes)
        assert int((pa < 0).sum()) == want_ptr[-1] - g.nnz and int((pb >= 0).sum()) == b.nnz, (mode, lanes)
        ref = [big.merge_row_reference(g, i, b.indices[b.indptr[i]:b.indptr[i + 1]], b.data[b.indptr[i]:b.indptr[i + 1]], mode) for i in m.rows]
        assert np.array_equal(out.col[pos].cpu().numpy(), np.concatenate([r[0] for r in ref]).astype(np.int32)), (mode, lanes)
        assert np.array_equal(out.val[pos].cpu().numpy().view(np.uint32), np.concatenate([r[1] for r in ref])), (mode, lanes)
        assert np.array_equal(pa[pos].cpu().numpy(), np.concatenate([r[2] for r in ref])), (mode, lanes)
        assert np.array_equal(pb[pos].cpu().numpy(), np.concatenate([np.where(r[3] >= 0, r[3] + b.indptr[i], -1) for i, r in zip(m.rows, ref)])), (mode, lanes)
        assert int(pa.max()) > m.bounds[-1]
        del out, pa, pb
        torch.cuda.empty_cache()
    print(f"[big csr] merge, tier {tier}, {len(runs)} runs: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("mode,lanes", [("sum", 0), ("keep", 4), ("keep", 16), ("sum", 64)])
def test_merge(cuda, mode, lanes):
    merge_case(cuda, "B", ((mode, lanes),))


# ---- select ----------------------------------------------------------------------------------------------------------------------------
def select_case(cuda, tier):
    m = matrix(cuda, "directed", tier)
    g = m.g
    t0 = time.perf_counter()
    rows = np.unique(m.rows)
    assert all(s in rows for s in (g.straddler(b) for b in m.bounds)) and (g.len[rows[g.rowptr[rows] > m.bounds[-1]]] > 2048).any()
    keep_rows = np.zeros(g.n, bool)
    keep_rows[rows] = True
    rmap, nr = csr_select_common.mask_to_map(keep_rows)
    keep_cols = np.arange(g.n) % 3 != 1
    cmap, nc = csr_select_common.mask_to_map(keep_cols)
    want = [g.row(i) for i in rows]
    hit = [keep_cols[w[0]] for w in want]
    want_ptr = np.concatenate(([0], np.cumsum([h.sum() for h in hit])))
    for lanes in (0, 4):
        out, pos = dev.csr_select(m.adj, row_map=torch.from_numpy(rmap).to(cuda), col_map=torch.from_numpy(cmap).to(cuda), n_rows_out=nr,
                                  n_cols_out=nc, lanes=lanes, positions=True)
        assert np.array_equal(out.rowptr.cpu().numpy(), want_ptr), lanes
        assert np.array_equal(out.col.cpu().numpy(), np.concatenate([cmap[w[0][h]] for w, h in zip(want, hit)])), lanes
        assert same_bits(out.val.cpu().numpy(), np.concatenate([w[1][h] for w, h in zip(want, hit)])), lanes
        assert np.array_equal(pos.cpu().numpy(), np.concatenate([w[2][h] for w, h in zip(want, hit)])) and int(pos.max()) > m.bounds[-1], lanes
    print(f"[big csr] select, tier {tier}: {time.perf_counter() - t0:.2f} s")


def test_select(cuda):
    select_case(cuda, "B")


# ---- one round of label propagation ----------------------------------------------------------------------------------------------------
def test_label_propagation_round(cuda):
    m = matrix(cuda, "directed", "B")
    g = m.g
    t0 = time.perf_counter()
    labels = ((np.arange(g.n) // 7) % 19).astype(np.int32)
    lab = torch.from_numpy(labels).to(cuda)
    for rnd, last in ((1, 0), (2, 1)):
        out = torch.full((g.n,), -1, dtype=torch.int32, device=cuda)
        moved = torch.zeros(1, dtype=torch.int64, device=cuda)
        dev._call(cuda, "sgl_reorder_lpa_round", ptr(m.rowptr), ptr(m.col), g.n, 0, g.n, ptr(lab), ptr(out), rnd, last, ptr(moved))
        assert int(out.min()) >= 0 and int(moved) == int((out != lab).sum()) > 0
        assert np.array_equal(out[m.rows_t].cpu().numpy(), big.lpa_rows_reference(g, m.rows, labels, rnd, last)), (rnd, last)
    print(f"[big csr] label propagation round: {time.perf_counter() - t0:.2f} s")


# ---- ingest ----------------------------------------------------------------------------------------------------------------------------
def test_ingest_in_transpose_order_with_pairs_stored_twice(cuda):
    """the entries of the directed matrix with rows and columns swapped, in the order A stores them -- for the result, A^T, that is
    no row-major order -- followed by every entry of the rows i % 1013 == 9 of A once more: those pairs are stored twice, in every
    part of the result.  Row j of the result is column j of A by formula; a pair stored twice is value + 0.25 in storage order."""
    m = matrix(cuda, "directed", "B")
    need(big.INGEST_NEED, "the ingest of tier B")
    g = m.g
    t0 = time.perf_counter()
    twice = np.arange(9, g.n, 1013)
    n_extra = int(g.len[twice].sum())
    total = g.nnz + n_extra
    assert big.B31 < total < (1 << 32) - 1
    in_row = torch.empty(total, dtype=torch.int64, device=cuda)
    in_col = torch.empty(total, dtype=torch.int64, device=cuda)
    in_val = torch.empty(total, dtype=torch.float32, device=cuda)
    in_row[:g.nnz] = m.col
    in_col[:g.nnz] = torch.repeat_interleave(torch.arange(g.n, dtype=torch.int64, device=cuda), torch.from_numpy(g.len).to(cuda))
    in_val[:g.nnz] = m.val
    pos = m.positions(g.rowptr, twice)
    in_row[g.nnz:] = m.col[pos]
    in_col[g.nnz:] = in_col[pos]
    in_val[g.nnz:] = 0.25
    del pos
    o_ptr = torch.full((g.n + 1,), -1, dtype=torch.int64, device=cuda)
    o_col = torch.full((total,), -1, dtype=torch.int32, device=cuda)
    o_val = torch.full((total,), NAN32, dtype=torch.float32, device=cuda)
    n_out = c_int64(0)
    t1 = time.perf_counter()
    dev._call(cuda, "sgl_coo_to_csr", g.n, g.n, total, ptr(in_row), ptr(in_col), ptr(in_val), ptr(o_ptr), ptr(o_col), ptr(o_val), ctypes.byref(n_out))
    t2 = time.perf_counter()
    del in_row, in_col, in_val
    want_ptr = torch.zeros(g.n + 1, dtype=torch.int64, device=cuda)
    want_ptr[1:] = torch.cumsum(big.column_lengths(g, cuda), 0)
    assert n_out.value == g.nnz and torch.equal(o_ptr, want_ptr)
    assert int(o_col[:g.nnz].min()) >= 0 and written(o_val[:g.nnz])
    pos = m.positions(want_ptr.cpu().numpy(), m.rows)
    assert int(pos.max()) > m.bounds[-1]
    ref = [g.column(j) for j in m.rows]
    vals = np.concatenate([np.where(r[0] % 1013 == 9, r[1] + np.float32(0.25), r[1]).astype(np.float32) for r in ref])
    assert (np.concatenate([r[0] for r in ref]) % 1013 == 9).sum() > 50
    assert np.array_equal(o_col[pos].cpu().numpy(), np.concatenate([r[0] for r in ref]).astype(np.int32))
    assert same_bits(o_val[pos].cpu().numpy(), vals)
    print(f"[big csr] ingest of {total} entries: {t2 - t1:.2f} s in the call, {time.perf_counter() - t0:.2f} s in all")


# ---- normalisation -----------------------------------------------------------------------------------------------------------------------
def check_norm_rows(m, rowptr_host, col, val, val64, ref, ulp=0):
    """the sampled rows of a normalised matrix against norm_rows_reference: columns, float32 bits (ulp = 0) and the fp64 values"""
    pos = m.positions(rowptr_host, m.rows)
    assert int(pos.max()) > m.bounds[-1]
    assert np.array_equal(col[pos].cpu().numpy(), np.concatenate([r[0] for r in ref]))
    want64 = np.concatenate([r[1] for r in ref])
    got = val[pos].cpu().numpy()
    if ulp == 0:
        assert same_bits(got, want64.astype(np.float32))
        assert val64 is None or same_bits(val64[pos].cpu().numpy(), want64)
    else:                                                   # the device's pow: the bar of test_gpu_norm_edges.check(bits32=False), and one ulp
        w32 = want64.astype(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - w32) <= ulp * np.spacing(np.abs(w32)).astype(np.float64))
        g64 = val64[pos].cpu().numpy()
        assert np.all(np.abs(g64 - want64) <= 1e-14 * np.abs(want64)) and not (g64 == 0).any()


def normalised_rowptr(m):
    """the row pointer of A_hat = the transposed A + I by formula: column lengths of A, and one more where A has no diagonal"""
    g = m.g
    ar = np.arange(g.n, dtype=np.int64)
    new = torch.from_numpy(g.find(ar, ar) < 0).to(m.cuda)
    out = torch.zeros(g.n + 1, dtype=torch.int64, device=m.cuda)
    out[1:] = torch.cumsum(big.column_lengths(g, m.cuda) + new, 0)
    return out, int(new.sum())


def norm_outputs(m, mm):
    n, cuda = m.g.n, m.cuda
    return (torch.full((n + 1,), -1, dtype=torch.int64, device=cuda), torch.full((mm,), -1, dtype=torch.int32, device=cuda),
            torch.full((mm,), NAN32, dtype=torch.float32, device=cuda), torch.full((mm,), NAN64, dtype=torch.float64, device=cuda))


def norm_whole_arrays(o, want_ptr):
    assert torch.equal(o[0], want_ptr) and int(o[1].min()) >= 0 and written(o[2]) and written(o[3])


def normalise_whole_matrix(cuda, kind):
    """sgl_norm_prepare, sgl_norm_degrees and sgl_norm_execute_lr (the sort-and-permute path with its 32-bit unsigned keys and
    positions, the host's degree powers: bit for bit), Laplacian and PPR"""
    m = matrix(cuda, kind, "B")
    need(big.NORM_NEED, "the whole-matrix normalisation of tier B")
    g = m.g
    n, nnz = g.n, g.nnz
    t0 = time.perf_counter()
    if kind == "symmetric":
        check_generated(m)
    want_ptr, want_ptr_host, n_new, lap, ppr = m.norm_references()
    nnz_out = c_int64(0)
    dev._call(cuda, "sgl_norm_prepare", n, nnz, ptr(m.rowptr), ptr(m.col), ctypes.byref(nnz_out))
    mm = nnz_out.value
    assert mm == nnz + n_new == want_ptr_host[-1] and n_new > 0
    deg = torch.full((n,), NAN64, dtype=torch.float64, device=cuda)
    dev._call(cuda, "sgl_norm_degrees", n, 0, ptr(m.rowptr), ptr(m.col), ptr(m.val), ptr(deg))
    assert written(deg) and same_bits(deg[m.rows_t].cpu().numpy(), np.array([big.row_degree(g, i) for i in m.rows]))
    print(f"[big csr] normalise {kind}: prepare, degrees and references {time.perf_counter() - t0:.2f} s")
    t0 = time.perf_counter()
    left, right = dev.degree_powers(deg, 0.5, host_pow=True)
    for use_alpha, alpha, ref in ((0, 0.0, lap), (1, 0.15, ppr)):
        o = norm_outputs(m, mm)
        dev._call(cuda, "sgl_norm_execute_lr", n, nnz, ptr(m.rowptr), ptr(m.col), ptr(m.val), ptr(left), ptr(right), use_alpha, alpha, mm,
                  *[ptr(t) for t in o])
        norm_whole_arrays(o, want_ptr)
        check_norm_rows(m, want_ptr_host, o[1], o[2], o[3], ref)
        del o
    print(f"[big csr] sgl_norm_execute_lr {kind}, Laplacian and PPR: {time.perf_counter() - t0:.2f} s")


def normalise_with_the_device_pow(cuda, kind):
    """sgl_norm_execute: the same path with the device's pow(), Laplacian and PPR"""
    m = matrix(cuda, kind, "B")
    need(big.NORM_NEED, "the whole-matrix normalisation of tier B")
    g = m.g
    want_ptr, want_ptr_host, n_new, lap, ppr = m.norm_references()
    mm = g.nnz + n_new
    t0 = time.perf_counter()
    for use_alpha, alpha, ref in ((0, 0.0, lap), (1, 0.15, ppr)):
        o = norm_outputs(m, mm)
        dev._call(cuda, "sgl_norm_execute", g.n, g.nnz, ptr(m.rowptr), ptr(m.col), ptr(m.val), 0.5, use_alpha, alpha, mm, *[ptr(t) for t in o])
        norm_whole_arrays(o, want_ptr)
        check_norm_rows(m, want_ptr_host, o[1], o[2], o[3], ref, ulp=1)
        del o
    print(f"[big csr] sgl_norm_execute {kind}, Laplacian and PPR: {time.perf_counter() - t0:.2f} s")


def prepared_adjacency(cuda, kind):
    """the route of the Python layer: sgl_norm_block_prepare, sgl_norm_build_symcheck, then for the symmetric matrix one scaling pass
    (sgl_norm_block_scale; the PPR mix through sgl_norm_block_diag_positions and sgl_norm_block_mix_at, whose grid cap of 2^22 blocks is
    passed here), for the directed one the transposition by sgl_coo_to_csr -- more than 2^31 entries in an order that is not row-major"""
    m = matrix(cuda, kind, "B")
    need(big.NORM_NEED, "the whole-matrix normalisation of tier B")
    g = m.g
    n = g.n
    want_ptr, want_ptr_host, n_new, lap, ppr = m.norm_references()
    mm = g.nnz + n_new
    t0 = time.perf_counter()
    prep = dev.PreparedAdjacency(m.rowptr, m.col, m.val, n)
    assert prep.symmetric == (kind == "symmetric") and prep.nnz_out == mm and not prep.may_hold_zero
    for alpha, ref in ((None, lap), (0.15, ppr)):
        got = prep.normalize(0.5, alpha, return_fp64=True)
        assert torch.equal(got[0], want_ptr) and int(got[1].min()) >= 0 and written(got[2])
        check_norm_rows(m, want_ptr_host, got[1], got[2], got[3], ref)
        del got
    if kind == "symmetric":
        HOLD["prep"] = prep
    print(f"[big csr] PreparedAdjacency, Laplacian and PPR: {time.perf_counter() - t0:.2f} s")


def test_normalise_whole_matrix_directed(cuda):
    normalise_whole_matrix(cuda, "directed")


def test_normalise_with_the_device_pow_directed(cuda):
    normalise_with_the_device_pow(cuda, "directed")


def test_prepared_adjacency_directed(cuda):
    prepared_adjacency(cuda, "directed")


def test_normalise_whole_matrix_symmetric(cuda):
    normalise_whole_matrix(cuda, "symmetric")


def test_normalise_with_the_device_pow_symmetric(cuda):
    normalise_with_the_device_pow(cuda, "symmetric")


def test_prepared_adjacency_symmetric(cuda):
    prepared_adjacency(cuda, "symmetric")


def test_normalise_row_blocks(cuda):
    """two row blocks of the symmetric matrix -- one that holds more than 2^31 entries itself, one whose first entry lies beyond
    2^31 of the whole matrix -- against the whole-matrix result: every bit of every row"""
    m = matrix(cuda, "symmetric", "B")
    need(big.NORM_NEED, "the row-block normalisation of tier B")
    g = m.g
    t0 = time.perf_counter()
    prep = HOLD.get("prep") or dev.PreparedAdjacency(m.rowptr, m.col, m.val, g.n)
    w_ptr, w_col, w_val, w_v64 = prep.normalize(0.5, 0.15, return_fp64=True)
    s = g.straddler(m.bounds[0])
    for a, e in ((0, s + 9), (s + 1, g.n)):
        p0, p1 = int(g.rowptr[a]), int(g.rowptr[e])
        assert (p1 - p0 > m.bounds[0]) if a == 0 else (p0 > m.bounds[0])
        rp = (m.rowptr[a:e + 1] - p0).contiguous()
        pb = dev.PreparedBlock(rp, m.col[p0:p1], m.val[p0:p1], a, g.n, symmetric=True, deg=prep.deg)
        got = pb.normalize(0.5, 0.15, return_fp64=True)
        q0, q1 = int(w_ptr[a]), int(w_ptr[e])
        assert torch.equal(got[0], w_ptr[a:e + 1] - q0) and torch.equal(got[1], w_col[q0:q1])
        assert torch.equal(got[2].view(torch.int32), w_val[q0:q1].view(torch.int32)) and torch.equal(got[3].view(torch.int64), w_v64[q0:q1].view(torch.int64))
        # sgl_norm_block_mix (the row-lookup form of the mix) from the cached fp64 Laplacian: the same bits
        hat = pb._hat64[1]
        o32 = torch.full((q1 - q0,), NAN32, dtype=torch.float32, device=cuda)
        dev._call(cuda, "sgl_norm_block_mix", e - a, a, ptr(pb.rowptr), ptr(pb.col), ptr(hat), 0.15, ptr(o32), None)
        assert torch.equal(o32.view(torch.int32), got[2].view(torch.int32))
        del o32, got
        if a == 0:                                          # sgl_norm_block_colsum over more than 2^31 entries (fp64 atomics: not bit-exact)
            cs = torch.zeros(g.n, dtype=torch.float64, device=cuda)
            dev._call(cuda, "sgl_norm_block_colsum", g.n, q1 - q0, ptr(pb.col), ptr(pb.t64), ptr(cs))
            ref = torch.zeros(g.n, dtype=torch.float64, device=cuda).index_add_(0, pb.col.long(), pb.t64)
            assert torch.allclose(cs, ref, rtol=1e-12, atol=0) and float(cs.max()) > 0
            del cs, ref
        del pb
        torch.cuda.empty_cache()
    HOLD.pop("prep", None)
    print(f"[big csr] row blocks: {time.perf_counter() - t0:.2f} s")


# ---- tier A: beyond 2^32, for the entry points without a cap there -----------------------------------------------------------------------
def test_tier_a_generated_matrix_is_the_formula(cuda):
    check_generated(matrix(cuda, "directed", "A"))


def test_tier_a_spmm(cuda):
    spmm_family(cuda, "A", "default")


def test_tier_a_find_and_candidates(cuda):
    find_case(cuda, "A")


def test_tier_a_permute_rows(cuda):
    permute_rows_case(cuda, "A")


def test_tier_a_select(cuda):
    select_case(cuda, "A")


def test_tier_a_merge(cuda):
    m = matrix(cuda, "directed", "A")
    if m.perm is not None:                                  # the permuted copy is not needed any more: make room for the position outputs
        m.perm = None
        torch.cuda.empty_cache()
    merge_case(cuda, "A", (("sum", 0),))

"""The CSR select on a real MI355X (csrc/sgl_csr_select.hip, device.csr_select, sgl_amd/transforms.py): run with `-m gpu`.

Everything here is integers and copied bits, so every comparison is exact: row pointer, columns, the bits of the values and the source
positions against the numpy oracle of csr_select_common (written from the predicate in include/sgl_hip.h), the public functions
against what the reference's transforms returned (tests/golden/g20_transforms.npz).  The raw entries are called on buffers with guard
words on either side of every output."""
import ctypes
from ctypes import c_int64, c_void_p

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import csr_select_common as common
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd import transforms as tr
from sgl_amd.io import DeviceAdjacency

pytestmark = pytest.mark.gpu

N_GUARD = 8
GUARDS = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A}
INT32_MAX = np.iinfo(np.int32).max


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


class Guarded:
    """n elements with N_GUARD guard elements on either side"""

    def __init__(self, n, dtype, cuda):
        self.n = n
        self.buf = torch.full((N_GUARD + n + N_GUARD,), GUARDS[dtype], dtype=dtype, device=cuda)
        self.ptr = c_void_p(self.buf.data_ptr() + N_GUARD * self.buf.element_size())

    def data(self):
        return self.buf[N_GUARD:N_GUARD + self.n].cpu().numpy()

    def intact(self):
        g = GUARDS[self.buf.dtype]
        return bool((self.buf[:N_GUARD] == g).all()) and bool((self.buf[N_GUARD + self.n:] == g).all())


def upload(a, cuda):
    """the arrays of a canonical scipy CSR on the device, bits untouched (from_scipy would canonicalise the NaNs away)"""
    return DeviceAdjacency(torch.from_numpy(a.indptr.astype(np.int64)).to(cuda), torch.from_numpy(a.indices.astype(np.int32)).to(cuda),
                           torch.from_numpy(a.data.astype(np.float32)).to(cuda), a.shape)


def raw_select(cuda, adj, lanes=0, row_map=None, col_map=None, n_rows_out=None, n_cols_out=None, entry_keep=None, symmetric_mask=False,
               drop_self=False, drop_below=0, seed=0, symmetric=False):
    """the two entries on guarded buffers: (rowptr, col, val, pos) as numpy arrays, sized exactly by the first call"""
    n_rows, n_cols = adj.shape
    nnz = adj.nnz
    keepalive = []

    def opt(x, dtype):
        if x is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dtype))).to(cuda)
        keepalive.append(t)
        return t

    rm, cm, ek = opt(row_map, np.int32), opt(col_map, np.int32), opt(entry_keep, np.uint8)
    before = [t.clone() for t in keepalive]
    n_rows_out = n_rows if row_map is None else n_rows_out
    n_cols_out = n_cols if col_map is None else n_cols_out
    col = adj.col if nnz else torch.zeros(1, dtype=torch.int32, device=cuda)
    val = adj.val if nnz else torch.zeros(1, dtype=torch.float32, device=cuda)
    sel = (dev._opt_ptr(rm), dev._opt_ptr(cm), n_rows_out, n_cols_out, dev._opt_ptr(ek), int(symmetric_mask), int(drop_self), int(drop_below),
           int(seed), int(symmetric), lanes)
    out_rowptr = Guarded(n_rows_out + 1, torch.int64, cuda)
    total = c_int64(-1)
    dev._call(cuda, "sgl_csr_select_rowptr", _lib.ptr(adj.rowptr), _lib.ptr(col), n_rows, n_cols, nnz, *sel, out_rowptr.ptr, ctypes.byref(total))
    m = total.value
    assert m >= 0 and out_rowptr.intact()
    out_col, out_val, out_pos = Guarded(m, torch.int32, cuda), Guarded(m, torch.int32, cuda), Guarded(m, torch.int64, cuda)
    dev._call(cuda, "sgl_csr_select_fill", _lib.ptr(adj.rowptr), _lib.ptr(col), _lib.ptr(val), n_rows, n_cols, nnz, *sel, out_rowptr.ptr, out_col.ptr,
              out_val.ptr, out_pos.ptr)
    torch.cuda.synchronize()
    assert out_rowptr.intact() and out_col.intact() and out_val.intact() and out_pos.intact()
    assert all(torch.equal(t, b) for t, b in zip(keepalive, before))                # the maps and the mask are only read
    rowptr = out_rowptr.data()
    assert rowptr[0] == 0 and rowptr[-1] == m and np.all(np.diff(rowptr) >= 0)
    return rowptr, out_col.data(), out_val.data().view(np.float32), out_pos.data()


def agrees(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and common.same_bits(got[2], want[2])
            and np.array_equal(got[3], want[3]))


def census(a, **kw):
    """(a row with entries of which none is kept, one of which all are kept, kept and dropped entries inside one stride of every
    instance: a row of at most 4 entries with both)"""
    keep, _, _ = common.oracle_keep(a.indptr, a.indices, a.shape[1], **kw)
    length = np.diff(a.indptr)
    kept = np.add.reduceat(np.concatenate((keep, [False])).astype(np.int64), np.minimum(a.indptr[:-1], len(keep)))
    kept[length == 0] = 0
    has = length > 0
    return bool((has & (kept == 0)).any()), bool((has & (kept == length)).any()), bool((has & (length <= 4) & (kept > 0) & (kept < length)).any())


@pytest.fixture(scope="module")
def rect():
    return common.zoo()


@pytest.fixture(scope="module")
def square():
    return common.zoo(n_rows=3001, n_cols=3001, seed=6, long_row=2000, mirror=0.5)


def threshold(p):
    return tr.drop_threshold(p)


def test_every_instance_over_the_zoo(cuda, rect):
    a = rect
    lengths = set(np.diff(a.indptr).tolist())
    assert a.shape == (6003, 7001) and a.shape[0] % 64 and a.shape[0] % 16 and a.shape[0] % 4
    for g in common.LANES:
        assert {0, 1, g - 1, g, g + 1} <= lengths, g
    assert {63, 64, 65, 5000} <= lengths and a.indptr[1] == 0 and a.indptr[-2] == a.indptr[-1]
    rng = np.random.RandomState(11)
    rmap, nr = common.mask_to_map(rng.rand(a.shape[0]) < 0.8)
    cmap, nc = common.mask_to_map(rng.rand(a.shape[1]) < 0.8)
    kw = dict(row_map=rmap, col_map=cmap, n_rows_out=nr, n_cols_out=nc, entry_keep=rng.rand(a.nnz) < 0.8, drop_below=threshold(0.2), seed=4)
    assert census(a, **kw) == (True, True, True)
    want = common.oracle_select(a, **kw)
    assert 0.3 * a.nnz < len(want[3]) < 0.7 * a.nnz
    adj = upload(a, cuda)
    first = None
    for lanes in (0,) + common.LANES:
        got = raw_select(cuda, adj, lanes=lanes, **kw)
        assert agrees(got, want), lanes
        again = raw_select(cuda, adj, lanes=lanes, **kw)
        assert all(common.same_bits(x, y) for x, y in zip(got, again)), lanes                  # a second run: the same bits
        first = first or got
        assert all(common.same_bits(x, y) for x, y in zip(got, first)), lanes                  # every instance: the same bits
    for bad in (1, 8, 32, 128, -4):
        with pytest.raises(ValueError, match="lanes"):
            dev.csr_select(adj, lanes=bad)
        with pytest.raises(_lib.SglHipError, match="sgl_csr_select_rowptr"):
            dev._call(cuda, "sgl_csr_select_rowptr", _lib.ptr(adj.rowptr), _lib.ptr(adj.col), a.shape[0], a.shape[1], a.nnz, None, None, a.shape[0],
                      a.shape[1], None, 0, 0, 0, 0, 0, bad, _lib.ptr(adj.rowptr), ctypes.byref(c_int64(0)))


def modes(a, square):
    rng = np.random.RandomState(12)
    n_rows, n_cols = a.shape
    rows, cols = rng.rand(n_rows) < 0.6, rng.rand(n_cols) < 0.5
    out = {}
    rmap, nr = common.mask_to_map(rows)
    cmap, nc = common.mask_to_map(cols)
    out["relabel, different row and column maps"] = dict(row_map=rmap, col_map=cmap, n_rows_out=nr, n_cols_out=nc)
    out["rows only"] = dict(row_map=rmap, n_rows_out=nr)
    out["columns only"] = dict(col_map=cmap, n_cols_out=nc)
    kmap, kn = common.mask_to_map(rows, keep_ids=True)
    kcmap, kc = common.mask_to_map(cols, keep_ids=True)
    out["identity or -1"] = dict(row_map=kmap, col_map=kcmap, n_rows_out=kn, n_cols_out=kc)
    out["entry mask"] = dict(entry_keep=rng.rand(a.nnz) < 0.5)
    out["drop_self"] = dict(drop_self=True)
    out["random"] = dict(drop_below=threshold(0.5), seed=21)
    out["random, symmetric"] = dict(drop_below=threshold(0.5), seed=22, symmetric=True)
    out["random, nearly all"] = dict(drop_below=threshold(1.0 - 2.0 ** -10), seed=23)
    if square:
        smap, sn = common.mask_to_map(rows)
        out["sub-graph"] = dict(row_map=smap, col_map=smap, n_rows_out=sn, n_cols_out=sn)
        out["symmetric mask"] = dict(entry_keep=rng.rand(a.nnz) < 0.5, symmetric_mask=True)
        out["all at once"] = dict(row_map=smap, col_map=smap, n_rows_out=sn, n_cols_out=sn, entry_keep=rng.rand(a.nnz) < 0.7, symmetric_mask=True,
                                  drop_self=True, drop_below=threshold(0.3), seed=24, symmetric=True)
    return out


@pytest.mark.parametrize("which", ["rect", "square"])
def test_each_mode_alone_and_all_at_once(cuda, rect, square, which):
    a = square if which == "square" else rect
    adj = upload(a, cuda)
    if which == "square":
        i = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
        stored = set(zip(i.tolist(), a.indices.tolist()))
        lower = [(r, c) for r, c in stored if c < r]
        assert sum((c, r) in stored for r, c in lower) > 1000 and sum((c, r) not in stored for r, c in lower) > 1000     # lower entries with and without a mirror
        assert sum(r == c for r, c in stored) > 100
    for name, kw in modes(a, which == "square").items():
        want = common.oracle_select(a, **kw)
        assert 0 < len(want[3]) < a.nnz, name
        if name in ("all at once", "entry mask", "random", "random, symmetric", "symmetric mask"):
            assert census(a, **kw) == (True, True, True), name
        for lanes in (0, 4, 64):
            assert agrees(raw_select(cuda, adj, lanes=lanes, **kw), want), (name, lanes)
        got, pos = dev.csr_select(adj, positions=True, **{k: (torch.from_numpy(np.ascontiguousarray(v)).to(cuda) if isinstance(v, np.ndarray) else v)
                                                            for k, v in kw.items()})
        assert agrees((got.rowptr.cpu().numpy(), got.col.cpu().numpy(), got.val.cpu().numpy(), pos.cpu().numpy()), want), name
        assert got.shape == (len(want[0]) - 1, kw.get("n_cols_out", a.shape[1]))


def test_everything_dropped_and_everything_kept(cuda, rect):
    a = rect
    adj = upload(a, cuda)
    for lanes in common.LANES:
        rowptr, col, val, pos = raw_select(cuda, adj, lanes=lanes)
        assert np.array_equal(rowptr, a.indptr) and np.array_equal(col, a.indices) and common.same_bits(val, a.data)
        assert np.array_equal(pos, np.arange(a.nnz))
        bits = set(val.view(np.uint32).tolist())
        assert {0x7FC01234, 0x80000000, 0x7F800000, 0x00000001} <= bits                       # NaN with its payload, -0.0, inf, a denormal
        assert np.isnan(val).sum() > 100
        for kw in (dict(entry_keep=np.zeros(a.nnz, bool)), dict(row_map=np.full(a.shape[0], -1, np.int32), n_rows_out=7),
                   dict(col_map=np.full(a.shape[1], -1, np.int32), n_cols_out=7), dict(row_map=np.full(a.shape[0], -1, np.int32), n_rows_out=0),
                   dict(col_map=np.full(a.shape[1], -1, np.int32), n_cols_out=0)):
            rowptr, col, val, pos = raw_select(cuda, adj, lanes=lanes, **kw)
            assert len(col) == 0 and not rowptr.any() and len(rowptr) == kw.get("n_rows_out", a.shape[0]) + 1
    same = dev.csr_select(adj)
    assert torch.equal(same.rowptr, adj.rowptr) and torch.equal(same.col, adj.col) and torch.equal(same.val.view(torch.int32), adj.val.view(torch.int32))
    none = dev.csr_select(adj, entry_keep=torch.zeros(a.nnz, dtype=torch.bool, device=cuda))
    assert none.nnz == 0 and none.shape == a.shape and not none.rowptr.any()


def test_hostile_map_values_are_dropped_and_nothing_is_written_outside(cuda, rect):
    a = rect
    adj = upload(a, cuda)
    rng = np.random.RandomState(13)
    rmap, nr = common.mask_to_map(rng.rand(a.shape[0]) < 0.5)
    cmap, nc = common.mask_to_map(rng.rand(a.shape[1]) < 0.5)
    want = common.oracle_select(a, row_map=rmap, col_map=cmap, n_rows_out=nr, n_cols_out=nc)
    for lanes in common.LANES:
        hr, hc = rmap.copy(), cmap.copy()
        hr[rmap < 0] = rng.choice([-2, nr, nr + 1, INT32_MAX, -INT32_MAX - 1, -1], size=int((rmap < 0).sum()))
        hc[cmap < 0] = rng.choice([-2, nc, nc + 5, INT32_MAX, -INT32_MAX - 1, -1], size=int((cmap < 0).sum()))
        assert (hr == INT32_MAX).any() and (hr == nr).any() and (hr == -2).any() and (hc == INT32_MAX).any() and (hc == nc).any()
        assert agrees(raw_select(cuda, adj, lanes=lanes, row_map=hr, col_map=hc, n_rows_out=nr, n_cols_out=nc), want), lanes


def test_no_entries_and_one_row(cuda):
    hollow = upload(sp.csr_matrix((5, 9), dtype=np.float32), cuda)
    for kw in ({}, dict(drop_self=True, drop_below=threshold(0.5)), dict(row_map=np.array([0, -1, 1, -1, 2], np.int32), n_rows_out=3)):
        rowptr, col, val, pos = raw_select(cuda, hollow, **kw)
        assert len(col) == 0 and not rowptr.any() and len(rowptr) == kw.get("n_rows_out", 5) + 1
    assert dev.csr_select(hollow).nnz == 0
    assert tr.remove_self_loops(hollow).shape == (5, 9)
    rng = np.random.RandomState(14)
    one = common.canonical(sp.csr_matrix((rng.rand(100).astype(np.float32) + 1, (np.zeros(100, int), np.sort(rng.choice(400, 100, replace=False)))),
                                         shape=(1, 400)))
    adj = upload(one, cuda)
    cmap, nc = common.mask_to_map(rng.rand(400) < 0.5)
    for lanes in (0,) + common.LANES:
        for kw in ({}, dict(entry_keep=rng.rand(100) < 0.5), dict(col_map=cmap, n_cols_out=nc), dict(drop_below=threshold(0.5), seed=3),
                   dict(row_map=np.array([-1], np.int32), n_rows_out=1), dict(row_map=np.array([2], np.int32), n_rows_out=4)):
            assert agrees(raw_select(cuda, adj, lanes=lanes, **kw), common.oracle_select(one, **kw)), (lanes, kw.keys())


# ---- the public functions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sym64", "pl256", "dir40", "symdiag48"])
def test_public_functions_against_the_reference(cuda, goldens, name):
    g = goldens.npz("g20_transforms")
    a = common.g20_graph(goldens, name)
    adj = DeviceAdjacency.from_scipy(a, device=cuda)
    edge_mask, node_mask = g[f"{name}|edge_mask"], g[f"{name}|node_mask"]
    rec = lambda key: common.recorded(goldens, f"{name}|{key}")      # noqa: E731
    dmask = torch.from_numpy(edge_mask).to(cuda)
    for fn in (tr.drop_edges, tr.biased_drop_edges):
        got = fn(adj, dmask)
        assert isinstance(got, DeviceAdjacency) and got.col.is_cuda and common.same_csr(got.to_scipy(), rec("drop"))
    assert common.same_csr(tr.drop_edges(a, edge_mask).to_scipy(), rec("drop"))                   # a scipy matrix is uploaded first
    assert common.same_csr(tr.remove_self_loops(adj).to_scipy(), rec("noself"))
    und = tr.drop_edges(adj, dmask, force_undirected=True).to_scipy()
    assert torch.equal(dmask.cpu(), torch.from_numpy(edge_mask))                                  # the mask is never written to
    assert common.same_csr(und, common.oracle_matrix(a, entry_keep=edge_mask, symmetric_mask=True))
    if name in ("sym64", "pl256"):
        assert common.same_csr(und, rec("drop_und"))
    x = np.random.RandomState(2).rand(a.shape[0], 5).astype(np.float32)
    y = np.arange(a.shape[0])
    dx = torch.from_numpy(x).to(cuda)
    sub = tr.get_subgraph(adj, node_mask, x=dx, y=y)
    assert common.same_csr(sub.adj.to_scipy(), rec("sub")) and common.same_csr(sub.adj.to_scipy(), a[node_mask][:, node_mask])
    assert np.array_equal(sub.x.cpu().numpy(), x[node_mask]) and np.array_equal(sub.y.cpu().numpy(), y[node_mask])
    assert np.array_equal(sub.node_ids.cpu().numpy(), np.nonzero(node_mask)[0])
    keep = tr.get_subgraph(adj, torch.from_numpy(node_mask), keep_ids=True, x=dx, y=y)
    assert common.same_csr(keep.adj.to_scipy(), rec("sub_keep")) and keep.adj.shape == a.shape
    assert np.array_equal(keep.x.cpu().numpy(), np.where(node_mask[:, None], x, 0)) and np.array_equal(dx.cpu().numpy(), x)   # a copy of x
    assert np.array_equal(keep.y.cpu().numpy(), y)
    for keep_ids, shape in ((False, (0, 0)), (True, a.shape)):
        empty = tr.get_subgraph(adj, np.zeros(a.shape[0], bool), keep_ids=keep_ids, x=dx)
        assert empty.adj.nnz == 0 and empty.adj.shape == shape and empty.node_ids.numel() == 0
        assert empty.x.shape == ((a.shape[0], 5) if keep_ids else (0, 5)) and not empty.x.any()
    with pytest.raises(ValueError, match="the shape of node mask is wrong!"):
        tr.get_subgraph(adj, node_mask[:-1])
    with pytest.raises(ValueError, match="the shape of edge drop mask is wrong!"):
        tr.drop_edges(adj, dmask[:-1])


@pytest.mark.parametrize("name", ["pl256", "dir40", "symdiag48"])
def test_random_drops_against_the_oracle(cuda, goldens, name):
    a = common.g20_graph(goldens, name)
    adj = DeviceAdjacency.from_scipy(a, device=cuda)
    for seed in (1, 2):
        for p in (0.5, 0.3):
            for und in (True, False):
                got = tr.random_drop_edges(adj, p=p, force_undirected=und, seed=seed).to_scipy()
                assert common.same_csr(got, common.oracle_matrix(a, drop_below=threshold(p), seed=seed, symmetric=und)), (seed, p, und)
                if und and name != "dir40":
                    assert (got != got.T).nnz == 0                                                  # a symmetric graph stays symmetric
        sub, mask = tr.random_drop_nodes(adj, p=0.4, seed=seed)
        m = common._hash4(seed, common.NODE_DROP_STREAM, np.arange(a.shape[0], dtype=np.uint64), np.uint64(0)) >= np.uint64(threshold(0.4))
        assert np.array_equal(mask.cpu().numpy(), m) and 0 < m.sum() < len(m)
        assert common.same_csr(sub.adj.to_scipy(), a[m][:, m])
        kept, mask2 = tr.random_drop_nodes(adj, p=0.4, seed=seed, keep_ids=True)
        ids, n_out = common.mask_to_map(m, keep_ids=True)
        assert torch.equal(mask, mask2) and common.same_csr(kept.adj.to_scipy(), common.oracle_matrix(a, row_map=ids, col_map=ids, n_rows_out=n_out, n_cols_out=n_out))
    assert tr.random_drop_edges(adj, p=0.0) is adj
    gone = tr.random_drop_edges(adj, p=1.0)
    assert gone.nnz == 0 and gone.shape == a.shape and gone.col.is_cuda
    nobody, mask = tr.random_drop_nodes(adj, p=1.0)
    assert nobody.adj.shape == (0, 0) and not mask.any()


def test_propagation_over_a_subgraph_is_bit_equal_to_the_scipy_route(cuda, goldens):
    from sgl_amd.operators.graph_op import LaplacianGraphOp
    a = common.canonical(goldens.graph("pl2000").astype(np.float32))
    n = a.shape[0]
    rng = np.random.RandomState(7)
    m = rng.rand(n) < 0.5
    x = torch.from_numpy(rng.randn(n, 24).astype(np.float32)).to(cuda)
    sub = tr.get_subgraph(DeviceAdjacency.from_scipy(a, device=cuda), m, x=x)
    assert torch.equal(sub.x, x[torch.from_numpy(m).to(cuda)])
    ours = LaplacianGraphOp(2).propagate(sub.adj, sub.x)
    theirs = LaplacianGraphOp(2).propagate(DeviceAdjacency.from_scipy(a[m][:, m], device=cuda), x[torch.from_numpy(m).to(cuda)])
    assert len(ours) == len(theirs) == 3
    for h, (u, v) in enumerate(zip(ours, theirs)):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), h


def test_positions_beyond_2_to_31(cuda):
    """2^31 + 2^20 entries generated on the device: 2^21 + 2^10 rows of 1024 entries, row i holding the columns 3 k + i % 3.  Rows with
    i % 101 == 7 and columns with c % 97 == 5 are kept, a share of about 10^-4; the value bits of entry p are p & 0x7FFFFFFF, so the
    kept set -- row pointer, columns, values, positions -- is known by formula."""
    free, _ = torch.cuda.mem_get_info()
    if free < 20 << 30:
        pytest.skip("needs 20 GiB of free device memory")
    width, n_rows, n_cols = 1024, (1 << 21) + (1 << 10), 3 * 1024 + 3
    nnz = n_rows * width
    assert nnz == (1 << 31) + (1 << 20)
    rowptr = torch.arange(n_rows + 1, dtype=torch.int64, device=cuda) * width
    col = torch.empty(nnz, dtype=torch.int32, device=cuda)
    val = torch.empty(nnz, dtype=torch.float32, device=cuda)
    k = torch.arange(width, dtype=torch.int64, device=cuda)
    col2, bits2 = col.view(n_rows, width), val.view(torch.int32).view(n_rows, width)
    step = 1 << 14
    for r0 in range(0, n_rows, step):
        i = torch.arange(r0, min(r0 + step, n_rows), dtype=torch.int64, device=cuda)
        col2[r0:r0 + step] = (3 * k[None, :] + (i % 3)[:, None]).to(torch.int32)
        bits2[r0:r0 + step] = ((i * width)[:, None] + k[None, :] & 0x7FFFFFFF).to(torch.int32)
    rows_kept = np.arange(n_rows) % 101 == 7
    cols_kept = np.arange(n_cols) % 97 == 5
    rmap, nr = common.mask_to_map(rows_kept)
    cmap, nc = common.mask_to_map(cols_kept)
    adj = DeviceAdjacency(rowptr, col, val, (n_rows, n_cols))
    out, pos = dev.csr_select(adj, row_map=torch.from_numpy(rmap).to(cuda), col_map=torch.from_numpy(cmap).to(cuda), n_rows_out=nr, n_cols_out=nc,
                              positions=True)
    i = np.nonzero(rows_kept)[0]
    c = 3 * np.arange(width)[None, :] + (i % 3)[:, None]                            # [kept rows, 1024]
    hit = cols_kept[c]
    want_pos = (i[:, None] * width + np.arange(width)[None, :])[hit]
    want_rowptr = np.concatenate(([0], np.cumsum(hit.sum(1))))
    assert 0.5e-4 < len(want_pos) / nnz < 2e-4 and want_pos.max() > (1 << 31)
    assert np.array_equal(out.rowptr.cpu().numpy(), want_rowptr)
    assert np.array_equal(pos.cpu().numpy(), want_pos)
    assert np.array_equal(out.col.cpu().numpy(), cmap[c[hit]])
    assert np.array_equal(out.val.view(torch.int32).cpu().numpy(), (want_pos & 0x7FFFFFFF).astype(np.int32))

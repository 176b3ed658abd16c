"""The CSR merge on a real MI355X (csrc/sgl_csr_merge.hip, device.csr_merge, sgl_amd/transforms.py add_edges / add_self_loops /
to_undirected): run with `-m gpu`.

Everything here is integers, copied bits and single float32 additions, so every comparison is exact: row pointer, columns, the bits
of the values and both position arrays against the numpy reference of csr_merge_common, the public functions against what the
reference's transforms returned (tests/golden/g22_merge_transforms.npz) under the stated condition (a pair that occurs three times
in the concatenation is compared with the model a + (b1 + b2), everything else with the golden).  The raw entries are called on
buffers with guard words on either side of every output."""
import ctypes
from ctypes import c_int64, c_void_p

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import csr_merge_common as common
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd import transforms as tr
from sgl_amd.io import DeviceAdjacency

pytestmark = pytest.mark.gpu

N_GUARD = 8
GUARDS = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A}
ZOO = common.shared_zoo()


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
    """the arrays of a scipy CSR on the device, bits untouched (from_scipy would canonicalise the NaNs away)"""
    return DeviceAdjacency(torch.from_numpy(a.indptr.astype(np.int64)).to(cuda), torch.from_numpy(a.indices.astype(np.int32)).to(cuda),
                           torch.from_numpy(a.data.astype(np.float32)).to(cuda), a.shape)


def raw_merge(cuda, a, b, lanes=0, mode=common.SUM, positions=True):
    """the two entries on guarded buffers, on the current stream: (rowptr, col, val, pos_a, pos_b) as numpy arrays, sized exactly by
    the first call"""
    n_rows, n_cols = a.shape
    one_i, one_f = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.float32, device=cuda)
    ca, va = (a.col, a.val) if a.nnz else (one_i, one_f)
    cb, vb = (b.col, b.val) if b.nnz else (one_i, one_f)
    before = [t.clone() for t in (a.rowptr, ca, va, b.rowptr, cb, vb)]
    out_rowptr = Guarded(n_rows + 1, torch.int64, cuda)
    total = c_int64(-1)
    dev._call(cuda, "sgl_csr_merge_rowptr", _lib.ptr(a.rowptr), _lib.ptr(ca), a.nnz, _lib.ptr(b.rowptr), _lib.ptr(cb), b.nnz, n_rows, n_cols, lanes,
              out_rowptr.ptr, ctypes.byref(total))
    m = total.value
    assert m >= 0 and out_rowptr.intact()
    out_col, out_val = Guarded(m, torch.int32, cuda), Guarded(m, torch.int32, cuda)
    pos_a, pos_b = Guarded(m, torch.int64, cuda), Guarded(m, torch.int64, cuda)
    dev._call(cuda, "sgl_csr_merge_fill", _lib.ptr(a.rowptr), _lib.ptr(ca), _lib.ptr(va), a.nnz, _lib.ptr(b.rowptr), _lib.ptr(cb), _lib.ptr(vb), b.nnz,
              n_rows, n_cols, mode, lanes, out_rowptr.ptr, out_col.ptr, out_val.ptr, pos_a.ptr if positions else None,
              pos_b.ptr if positions else None)
    torch.cuda.current_stream().synchronize()
    assert out_rowptr.intact() and out_col.intact() and out_val.intact() and pos_a.intact() and pos_b.intact()
    assert all(torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, u.view(torch.int32) if u.dtype == torch.float32 else u)
               for t, u in zip((a.rowptr, ca, va, b.rowptr, cb, vb), before))       # the inputs are only read
    rowptr = out_rowptr.data()
    assert rowptr[0] == 0 and rowptr[-1] == m and np.all(np.diff(rowptr) >= 0)
    if not positions:
        assert bool((pos_a.buf == GUARDS[torch.int64]).all()) and bool((pos_b.buf == GUARDS[torch.int64]).all())
    return rowptr, out_col.data(), out_val.data().view(np.float32), pos_a.data(), pos_b.data()


@pytest.fixture(scope="module")
def wanted():
    """the numpy reference of every zoo case and mode, computed once"""
    return {(case, mode): common.merge_reference(a, b, mode) for case, (a, b) in ZOO.items() for mode in (common.SUM, common.KEEP)}


@pytest.mark.parametrize("case", sorted(ZOO))
def test_every_instance_and_mode_over_the_zoo(cuda, wanted, case):
    a, b = ZOO[case]
    da, db = upload(a, cuda), upload(b, cuda)
    side = torch.cuda.Stream(device=cuda)
    for mode in (common.SUM, common.KEEP):
        want = wanted[(case, mode)]
        first = None
        for lanes in (0,) + common.LANES:
            got = raw_merge(cuda, da, db, lanes=lanes, mode=mode)
            assert common.agrees(got, want), (mode, lanes)
            first = first or got
            assert all(common.same_bits(x, y) for x, y in zip(got, first)), (mode, lanes)      # every instance: the same bytes
        torch.cuda.synchronize()
        with torch.cuda.stream(side):                                                          # the same on a side stream
            got = raw_merge(cuda, da, db, lanes=16, mode=mode)
        side.synchronize()
        assert all(common.same_bits(x, y) for x, y in zip(got, first)), mode
        plain = raw_merge(cuda, da, db, lanes=4, mode=mode, positions=False)                   # both position outputs are optional
        assert all(common.same_bits(x, y) for x, y in zip(plain[:3], first[:3])), mode
    out, (pa, pb) = dev.csr_merge(da, db, mode="keep", positions=True)
    got = (out.rowptr.cpu().numpy(), out.col.cpu().numpy(), out.val.cpu().numpy(), pa.cpu().numpy(), pb.cpu().numpy())
    assert common.agrees(got, wanted[(case, common.KEEP)]) and out.shape == a.shape
    out = dev.csr_merge(da, db)
    assert common.agrees((out.rowptr.cpu().numpy(), out.col.cpu().numpy(), out.val.cpu().numpy()) + got[3:], wanted[(case, common.SUM)])


def test_special_values_survive(cuda, wanted):
    a, b = ZOO["main"]
    got = raw_merge(cuda, upload(a, cuda), upload(b, cuda), mode=common.SUM)
    bits = set(got[2].view(np.uint32).tolist())
    assert {0x7FC01234, 0xFFC0ABCD, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x00000002} <= bits
    a, b = ZOO["square"]
    got = raw_merge(cuda, upload(a, cuda), upload(b, cuda), mode=common.SUM)
    assert ((got[3] >= 0) & (got[4] >= 0) & (got[2] == 0)).sum() >= 10                         # a zero sum stays stored


def test_bad_arguments_are_errors_and_the_next_good_call_is_right(cuda, wanted):
    a, b = ZOO["square"]
    da, db = upload(a, cuda), upload(b, cuda)
    other = upload(ZOO["tall"][0], cuda)
    for bad in (1, 8, 32, 128, -4):
        with pytest.raises(ValueError, match="lanes"):
            dev.csr_merge(da, db, lanes=bad)
        with pytest.raises(_lib.SglHipError, match="sgl_csr_merge_rowptr"):
            dev._call(cuda, "sgl_csr_merge_rowptr", _lib.ptr(da.rowptr), _lib.ptr(da.col), da.nnz, _lib.ptr(db.rowptr), _lib.ptr(db.col), db.nnz,
                      a.shape[0], a.shape[1], bad, _lib.ptr(torch.empty(a.shape[0] + 1, dtype=torch.int64, device=cuda)), ctypes.byref(c_int64(0)))
    with pytest.raises(_lib.SglHipError, match="sgl_csr_merge_fill"):
        dev._call(cuda, "sgl_csr_merge_fill", _lib.ptr(da.rowptr), _lib.ptr(da.col), _lib.ptr(da.val), da.nnz, _lib.ptr(db.rowptr), _lib.ptr(db.col),
                  _lib.ptr(db.val), db.nnz, a.shape[0], a.shape[1], 2, 0, _lib.ptr(da.rowptr), _lib.ptr(da.col), _lib.ptr(da.val), None, None)
    with pytest.raises(ValueError, match="mode"):
        dev.csr_merge(da, db, mode="max")
    with pytest.raises(ValueError, match="shapes differ"):
        dev.csr_merge(da, other)
    short = DeviceAdjacency(da.rowptr, da.col[:-1], da.val[:-1], da.shape)
    with pytest.raises(ValueError, match="rowptr ends at"):
        dev.csr_merge(short, db)
    with pytest.raises(ValueError, match="rowptr ends at"):
        dev.csr_merge(da, DeviceAdjacency(db.rowptr, db.col[:-1], db.val[:-1], db.shape))
    with pytest.raises(TypeError):
        dev.csr_merge(da, DeviceAdjacency(db.rowptr, db.col, db.val.double(), db.shape))
    with pytest.raises(TypeError):
        dev.csr_merge(da, DeviceAdjacency(db.rowptr.cpu(), db.col.cpu(), db.val.cpu(), db.shape))
    with pytest.raises(TypeError):
        dev.csr_merge(DeviceAdjacency(da.rowptr.to(torch.int32), da.col, da.val, da.shape), db)
    assert common.agrees(raw_merge(cuda, da, db), wanted[("square", common.SUM)])


def test_a_row_that_is_not_sorted_is_survived(cuda):
    """An input the contract forbids and the kernel must survive: one row of B unsorted.  No error, nothing outside the outputs is
    written (the guard words are checked inside raw_merge), the row pointer still adds up, and every other row is right."""
    a, b = ZOO["main"]
    i = int(np.argmax((np.diff(b.indptr) == 65) & (np.diff(a.indptr) == 64)))
    hostile = b.copy()
    s, e = hostile.indptr[i], hostile.indptr[i + 1]
    hostile.indices[s:e] = hostile.indices[s:e][::-1].copy()
    want = common.merge_reference(a, b)
    for lanes in common.LANES:
        for mode in (common.SUM, common.KEEP):
            got = raw_merge(cuda, upload(a, cuda), upload(hostile, cuda), lanes=lanes, mode=mode)
            assert np.all(np.diff(got[0]) >= 0) and np.all(np.diff(got[0]) <= np.diff(a.indptr) + np.diff(b.indptr))
            rows = np.repeat(np.arange(a.shape[0]), np.diff(got[0]))
            rows_want = np.repeat(np.arange(a.shape[0]), np.diff(want[0]))
            assert np.array_equal(got[1][rows != i], want[1][rows_want != i])


# ---- the public functions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", common.G22_GRAPHS)
def test_public_functions_against_the_reference(cuda, goldens, name):
    g = goldens.npz("g22_merge_transforms")
    a = common.g22_graph(goldens, name)
    n = a.shape[0]
    adj = DeviceAdjacency.from_scipy(a, device=cuda)
    idx, w = g[f"{name}|add_idx"], g[f"{name}|add_w"]
    rec = lambda key: common.recorded(goldens, f"{name}|{key}")      # noqa: E731
    for indices, weights in ((torch.from_numpy(idx).to(cuda), torch.from_numpy(w).to(cuda)), (torch.from_numpy(idx), torch.from_numpy(w)),
                             (idx, w), (idx.tolist(), w.tolist()), (idx.astype(np.int32), torch.from_numpy(w).to(cuda))):
        got = tr.add_edges(adj, indices, weights)
        assert isinstance(got, DeviceAdjacency) and got.col.is_cuda and got.shape == a.shape
        common.check_against_add_golden(got.to_scipy(), a, idx, w, rec("add"))
        common.check_against_del_golden(tr.add_edges(adj, indices, weights, del_repeated=True).to_scipy(), a, idx, w, rec("add_del"))
    common.check_against_add_golden(tr.add_edges(a, idx, w).to_scipy(), a, idx, w, rec("add"))           # a scipy matrix is uploaded first
    ones = tr.add_edges(adj, idx)                                                                        # weights default to ones
    model = common.merge_reference(a, common.storage_order_csr(idx, np.ones(idx.shape[1], dtype=np.float32), a.shape))
    assert np.array_equal(ones.rowptr.cpu().numpy(), model[0]) and np.array_equal(ones.col.cpu().numpy(), model[1])
    assert common.same_bits(ones.val.cpu().numpy(), model[2])
    assert tr.add_edges(adj, torch.zeros(2, 0, dtype=torch.int64, device=cuda)) is adj
    with pytest.raises(ValueError, match=r"indices must be in range of \[0, num_node\)!"):
        tr.add_edges(adj, torch.tensor([[0, n], [1, 2]], device=cuda))
    loop_w = g[f"{name}|loop_w"]
    for got, key in ((tr.add_self_loops(adj), "loops"), (tr.add_self_loops(adj, loop_w), "loops_w"),
                     (tr.add_self_loops(adj, torch.from_numpy(loop_w).to(cuda)), "loops_w"), (tr.add_self_loops(a, loop_w.tolist()), "loops_w")):
        want = rec(key)
        m = got.to_scipy()
        assert np.array_equal(m.indptr, want.indptr) and np.array_equal(m.indices, want.indices) and common.same_bits(m.data, want.data), key
        assert np.array_equal(m.diagonal(), a.diagonal() + (loop_w if key == "loops_w" else 1))
    stored_diagonal = np.count_nonzero(common.keys(a) % (n + 1) == 0)
    assert tr.add_self_loops(adj).nnz == a.nnz + n - stored_diagonal
    if name == "symdiag48":
        assert 10 < stored_diagonal < n                                                                  # a partly stored diagonal
    und = tr.to_undirected(adj).to_scipy()
    want = rec("und")
    assert np.array_equal(und.indptr, want.indptr) and np.array_equal(und.indices, want.indices) and common.same_bits(und.data, want.data)
    assert np.array_equal(adj.val.cpu().numpy(), a.data)                                                 # the input is only read


def test_to_undirected_of_a_directed_graph(cuda, goldens):
    a = common.g22_graph(goldens, "dir40")
    adj = DeviceAdjacency.from_scipy(a, device=cuda)
    coo = a.tocoo()
    doubled = sp.csr_matrix((np.concatenate((coo.data, coo.data)), (np.concatenate((coo.row, coo.col)), np.concatenate((coo.col, coo.row)))),
                            shape=a.shape)                                                               # the reference's way
    doubled.sum_duplicates()
    doubled.sort_indices()
    got = tr.to_undirected(adj, reduce="sum").to_scipy()
    assert np.array_equal(got.indptr, doubled.indptr) and np.array_equal(got.indices, doubled.indices) and common.same_bits(got.data, doubled.data)
    structure = sp.csr_matrix((np.ones(got.nnz), got.indices, got.indptr), shape=got.shape)
    assert (structure != structure.T).nnz == 0 and got.nnz > a.nnz                                       # symmetric in structure
    from sgl_amd.io import coo_to_csr_device
    rows = torch.repeat_interleave(torch.arange(a.shape[0], device=cuda), adj.rowptr[1:] - adj.rowptr[:-1])
    mirror = coo_to_csr_device(adj.col.to(torch.int64), rows, adj.val, a.shape[0], device=cuda)
    kept, (pa, pb) = dev.csr_merge(adj, mirror, mode="keep", positions=True)
    pub = tr.to_undirected(adj, reduce="keep")
    assert torch.equal(pub.rowptr, kept.rowptr) and torch.equal(pub.col, kept.col) and torch.equal(pub.val.view(torch.int32), kept.val.view(torch.int32))
    assert np.array_equal(pub.col.cpu().numpy(), doubled.indices)
    stored = pa >= 0
    assert int(stored.sum()) == a.nnz and torch.equal(pa[stored], torch.arange(a.nnz, device=cuda))
    assert torch.equal(pub.val[stored].view(torch.int32), adj.val.view(torch.int32))                     # every stored value: its bits unchanged
    filled = ~stored
    assert torch.equal(pub.val[filled].view(torch.int32), mirror.val[pb[filled]].view(torch.int32)) and int(filled.sum()) == got.nnz - a.nnz
    hollow = DeviceAdjacency(torch.zeros(6, dtype=torch.int64, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda),
                             torch.zeros(0, dtype=torch.float32, device=cuda), (5, 5))
    assert tr.to_undirected(hollow) is hollow and tr.add_self_loops(hollow).nnz == 5


def test_propagation_over_an_undirected_graph_is_bit_equal_to_the_scipy_route(cuda, goldens):
    from sgl_amd.operators.graph_op import LaplacianGraphOp
    a = common.g22_graph(goldens, "pl256")
    n = a.shape[0]
    coo = a.tocoo()
    doubled = sp.csr_matrix((np.concatenate((coo.data, coo.data)), (np.concatenate((coo.row, coo.col)), np.concatenate((coo.col, coo.row)))),
                            shape=a.shape)
    x = torch.from_numpy(np.random.RandomState(8).randn(n, 7).astype(np.float32)).to(cuda)
    ours = LaplacianGraphOp(3).propagate(tr.to_undirected(DeviceAdjacency.from_scipy(a, device=cuda)), x)
    theirs = LaplacianGraphOp(3).propagate(DeviceAdjacency.from_scipy(doubled, device=cuda), x)
    assert len(ours) == len(theirs) == 4
    for h, (u, v) in enumerate(zip(ours, theirs)):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), h


def test_loader_option(cuda, tmp_path, goldens):
    from sgl_amd import io
    a = common.g22_graph(goldens, "dir40")
    coo = a.tocoo()
    np.savez(tmp_path / "adj_matrix.npz", row=coo.row, col=coo.col, data=coo.data)
    plain = io.load_custom_homo_raw(str(tmp_path), num_node=40, device=cuda)["adj"]
    assert plain.nnz == a.nnz
    adj = DeviceAdjacency.from_scipy(a, device=cuda)
    for how in ("sum", "keep"):
        got = io.load_custom_homo_raw(str(tmp_path), num_node=40, device=cuda, undirected=how)["adj"]
        want = tr.to_undirected(adj, reduce=how)
        assert torch.equal(got.rowptr, want.rowptr) and torch.equal(got.col, want.col) and torch.equal(got.val.view(torch.int32), want.val.view(torch.int32))


def test_medium_graph_against_a_torch_composition(cuda):
    """About 200 000 nodes and 2 M entries merged with 100 000 random pairs (a tenth of them stored pairs, some repeated): structure
    exact, values exact wherever the pair occurs at most twice in the concatenation (one float32 addition commutes)."""
    n, m, x = 200_003, 2_000_000, 100_000
    gen = torch.Generator(device=cuda)
    gen.manual_seed(5)
    key = torch.unique(torch.randint(0, n * n, (m + m // 8,), device=cuda, generator=gen))[:m]
    val = torch.rand(key.numel(), device=cuda, generator=gen) + 0.5
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=cuda)
    rowptr[1:] = torch.cumsum(torch.bincount(key // n, minlength=n), 0)
    adj = DeviceAdjacency(rowptr, (key % n).to(torch.int32), val, (n, n))
    stored = key[torch.randint(0, key.numel(), (x // 10,), device=cuda, generator=gen)]
    fresh = torch.randint(0, n * n, (x - x // 10 - 100,), device=cuda, generator=gen)
    add = torch.cat((stored, fresh, fresh[:100]))                                      # 100 pairs listed twice
    add = add[torch.randperm(add.numel(), device=cuda, generator=gen)]
    w = torch.rand(add.numel(), device=cuda, generator=gen) - 0.5
    got = tr.add_edges(adj, torch.stack((add // n, add % n)), w)
    every = torch.cat((key, add))
    uniq, inverse, count = torch.unique(every, return_inverse=True, return_counts=True)
    total = torch.zeros(uniq.numel(), dtype=torch.float32, device=cuda).index_add_(0, inverse, torch.cat((val, w)))
    want_rowptr = torch.zeros(n + 1, dtype=torch.int64, device=cuda)
    want_rowptr[1:] = torch.cumsum(torch.bincount(uniq // n, minlength=n), 0)
    assert got.nnz == uniq.numel() and torch.equal(got.rowptr, want_rowptr) and torch.equal(got.col, (uniq % n).to(torch.int32))
    few = count <= 2
    assert int((count == 2).sum()) > x // 20 and int(few.sum()) > m
    assert torch.equal(got.val[few].view(torch.int32), total[few].view(torch.int32))
    kept = tr.add_edges(adj, torch.stack((add // n, add % n)), w, del_repeated=True)
    assert torch.equal(kept.rowptr, want_rowptr) and torch.equal(kept.col, got.col)
    at = torch.searchsorted(uniq, key)
    assert torch.equal(kept.val[at].view(torch.int32), val.view(torch.int32))          # the stored value always wins

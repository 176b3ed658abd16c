"""The sparse x sparse product on a real MI355X (csrc/sgl_spgemm.hip, device.csr_matmul; include/sgl_spgemm.h): run with `-m gpu`.

Every case is multiplied under every forcing of the row classes and of the bitmap window, and the results must be the same bytes.
References are scipy's: the pattern is that of the float64 product of the stored patterns (positive, so nothing is pruned);
values="sum" is bit-equal to scipy's sorted float32 product on positive inputs and within (L + 1) 2^-24 sum|a b| of the float64
product, L the entry's number of products (the bound of an L-term ordered float32 sum); values="ones" is 1.0 everywhere."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.io import DeviceAdjacency

pytestmark = pytest.mark.gpu

# (narrow_cap, window_cols): auto; everything but the smallest rows through the bitmap, several windows per row; each larger slice
FORCINGS = ((0, 0), (32, 1024), (128, 1024), (512, 1024), (32, 32768))


def sparse(rng, m, k, density):
    """[m, k] float32 CSR, values in [0.5, 1.5); density: a number or one per row"""
    keep = rng.random((m, k)) < np.reshape(density, (-1, 1))
    return sp.csr_matrix(np.where(keep, rng.random((m, k)) + 0.5, 0).astype(np.float32))


def lengths(k, lens, hit):
    """[len(lens), k] float32 CSR whose row r stores its first lens[r] columns; [k, n] with one entry per row, row j at column hit(j)"""
    a = sp.csr_matrix((np.arange(k)[None, :] < np.reshape(lens, (-1, 1))).astype(np.float32) * 0.75)
    cols = np.array([hit(j) for j in range(k)])
    b = sp.csr_matrix((np.linspace(0.5, 1.5, k, dtype=np.float32), (np.arange(k), cols)), shape=(k, int(cols.max()) + 1))
    return a, b


def make_cases():
    rng = np.random.default_rng(17)
    cases = {}
    # rectangular, 600 rows (more than one workgroup covers in any class): rows from empty to ~20 entries, empty rows of B, rows of A
    # that meet only those (ub = 0), columns 0 and n - 1 stored, n past one window
    a, b = sparse(rng, 600, 53, (np.arange(600) % 10) ** 2 / 200).tolil(), sparse(rng, 53, 1500, 0.005).tolil()
    b[[3, 17, 52]] = 0
    a[5], a[6] = 0, 0
    a[5, 3], a[6, 17], a[6, 52], b[0, 0], b[51, 1499] = 1.0, 1.0, 1.0, 1.25, 0.625
    cases["rect"] = (a.tocsr(), b.tocsr())
    for x in cases["rect"]:
        x.eliminate_zeros()
    # a row's bound at every slice size and one above: the slice filled to its last key, and the same row from the next class; every
    # column of C is reached many times
    cases["slice_edges"] = lengths(513, [32, 33, 128, 129, 512, 513, 1, 0], lambda j: j % 29)
    # one run holds everything: every candidate of every row is column 7, reached through every entry of A's row
    cases["one_column"] = lengths(200, [200, 40, 3, 150], lambda j: 7)
    # a full row over a fairly dense B: more distinct columns than one window holds; bits on both sides of a 32-bit word, a 64-bit word
    # and a window edge; n equal to the window and one more
    for n in (1024, 1025, 2500):
        a, b = sparse(rng, 3, 40, [1.0, 0.5, 0.02]), sparse(rng, 40, n, 0.1).tolil()
        for c in (0, 31, 32, 63, 64, 1023, 1024, n - 1):
            if c < n:
                b[0, c] = 0.875
        cases[f"full_row_{n}"] = (a, b.tocsr())
    z = sp.csr_matrix((4, 6), dtype=np.float32)
    cases["a_empty"], cases["b_empty"] = (z, sparse(rng, 6, 9, 0.5)), (sparse(rng, 5, 4, 0.5), z)
    cases["no_rows"] = (sp.csr_matrix((0, 6), dtype=np.float32), sparse(rng, 6, 9, 0.5))
    return cases


CASES = make_cases()


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def wanted():
    """per case: the sorted float64 product of the patterns (its values: products per entry), the float64 and the sorted float32 product"""
    out = {}
    for name, (a, b) in CASES.items():
        ones = lambda x: sp.csr_matrix((np.ones(x.nnz), x.indices, x.indptr), shape=x.shape)      # noqa: E731
        pattern, exact, single = ones(a) @ ones(b), a.astype(np.float64) @ b.astype(np.float64), a @ b
        for x in (pattern, exact, single):
            x.sort_indices()
        assert single.dtype == np.float32 and single.nnz == pattern.nnz == exact.nnz
        out[name] = (pattern, exact, single)
    return out


def upload(x, cuda):
    x = sp.csr_matrix(x)
    x.sort_indices()
    return DeviceAdjacency(torch.from_numpy(x.indptr.astype(np.int64)).to(cuda), torch.from_numpy(x.indices.astype(np.int32)).to(cuda),
                           torch.from_numpy(x.data.astype(np.float32)).to(cuda), x.shape)


def arrays(c):
    return c.rowptr.cpu().numpy(), c.col.cpu().numpy(), c.val.cpu().numpy()


@pytest.mark.parametrize("values", ["sum", "ones"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_forcing_gives_the_reference_and_the_same_bytes(cuda, wanted, case, values):
    a, b = (upload(x, cuda) for x in CASES[case])
    pattern, exact, single = wanted[case]
    first = None
    for narrow_cap, window_cols in FORCINGS:
        c = dev.csr_matmul(a, b, values=values, narrow_cap=narrow_cap, window_cols=window_cols)
        rowptr, col, val = arrays(c)
        assert c.shape == pattern.shape and c.nnz == pattern.nnz, (narrow_cap, window_cols)
        assert np.array_equal(rowptr, pattern.indptr) and np.array_equal(col, pattern.indices), (narrow_cap, window_cols)
        if values == "ones":
            assert np.array_equal(val, np.ones(c.nnz, dtype=np.float32))
        else:
            assert np.array_equal(val.view(np.uint32), single.data.view(np.uint32)), (narrow_cap, window_cols)
            assert np.all(np.abs(val.astype(np.float64) - exact.data) <= (pattern.data + 1) * 2.0 ** -24 * exact.data)
        first = first or (rowptr, col, val)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip((rowptr, col, val), first)), (narrow_cap, window_cols)
    if case == "rect":                                                          # one workgroup per kernel: every list is strided over
        _lib.set_tuning("spgemm_blocks", 1)
        try:
            for narrow_cap in (32, 512):
                got = arrays(dev.csr_matmul(a, b, values=values, narrow_cap=narrow_cap, window_cols=1024))
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, first)), narrow_cap
        finally:
            _lib.set_tuning("spgemm_blocks", 0)


def test_the_cases_hold_what_they_promise(wanted):
    bound = lambda a, b: np.asarray(sp.csr_matrix((np.ones(a.nnz), a.indices, a.indptr), shape=a.shape) @ np.diff(b.indptr))   # noqa: E731
    ub = bound(*CASES["rect"])
    assert ub[5] == ub[6] == 0 and CASES["rect"][0][5].nnz == 1 and (np.diff(CASES["rect"][0].indptr) == 0).sum() > 60
    for lo, hi, rows in ((1, 32, 64), (33, 128, 16), (129, 512, 4)):            # more rows in every class than one workgroup takes
        assert ((ub >= lo) & (ub <= hi)).sum() > rows
    assert (ub > 32).sum() > 64 and {0, 1499} <= set(wanted["rect"][0].indices.tolist())
    assert bound(*CASES["slice_edges"]).tolist() == [32, 33, 128, 129, 512, 513, 1, 0]
    assert set(wanted["one_column"][0].indices.tolist()) == {7} and wanted["one_column"][0].data.max() == 200
    for n in (1024, 1025, 2500):
        row = wanted[f"full_row_{n}"][0][0].indices
        assert {0, 31, 32, 63, 64, 1023, n - 1} <= set(row.tolist()) and (n < 2500 or row.size > 2048)


def test_a_zero_sum_stays_stored(cuda):
    """the documented difference from scipy, which prunes the cancelled entry"""
    a = np.array([[1, -1], [2, 3]], dtype=np.float32)
    b = np.array([[1, 0], [1, 5]], dtype=np.float32)
    assert (sp.csr_matrix(a) @ sp.csr_matrix(b)).nnz == 3
    for narrow_cap in (0, 32):
        rowptr, col, val = arrays(dev.csr_matmul(upload(a, cuda), upload(b, cuda), narrow_cap=narrow_cap))
        assert rowptr.tolist() == [0, 2, 4] and col.tolist() == [0, 1, 0, 1] and val.tolist() == [0.0, -5.0, 5.0, 15.0]


def test_bad_arguments_are_errors(cuda):
    a, b = (upload(x, cuda) for x in CASES["rect"])
    with pytest.raises(ValueError, match="do not chain"):
        dev.csr_matmul(a, a)
    for bad in (1, 64, 1024):
        with pytest.raises(ValueError, match="narrow_cap"):
            dev.csr_matmul(a, b, narrow_cap=bad)
        with pytest.raises(_lib.SglHipError, match="sgl_csr_matmul_rowptr: narrow_cap"):
            dev._call(cuda, "sgl_csr_matmul_rowptr", _lib.ptr(a.rowptr), _lib.ptr(a.col), a.nnz, _lib.ptr(b.rowptr), _lib.ptr(b.col), b.nnz, 600, 53,
                      1500, bad, 0, _lib.ptr(torch.empty(601, dtype=torch.int64, device=cuda)), None)
    with pytest.raises(ValueError, match="window_cols"):
        dev.csr_matmul(a, b, window_cols=2048)
    with pytest.raises(ValueError, match="values"):
        dev.csr_matmul(a, b, values="max")

"""What the CSR-select tests share (csrc/sgl_csr_select.hip, device.csr_select, sgl_amd/transforms.py): a numpy oracle of the
predicate that include/sgl_hip.h states -- written from that text, with sgl_amd/synthetic.py's mirror of the counter hash -- and the
matrices the kernels are run on."""
import numpy as np
import scipy.sparse as sp

from sgl_amd.synthetic import _hash4
from sgl_amd.transforms import drop_threshold  # noqa: F401  (the tests' thresholds; pinned exactly in test_csr_select_cpu.test_threshold_is_exact)

EDGE_DROP_STREAM, NODE_DROP_STREAM = 103, 104
LANES = (4, 16, 64)


def canonical(a):
    a = sp.csr_matrix(a)
    a.sum_duplicates()
    a.sort_indices()
    return a


def oracle_keep(indptr, indices, n_cols, row_map=None, col_map=None, n_rows_out=None, n_cols_out=None, entry_keep=None,
                symmetric_mask=False, drop_self=False, drop_below=0, seed=0, symmetric=False):
    """(keep bool [nnz], out_row int64 [nnz], out_col int64 [nnz]) of every source entry, in entry order"""
    indptr = np.asarray(indptr, dtype=np.int64)
    n_rows = len(indptr) - 1
    nnz = int(indptr[-1])
    i = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(indptr))
    j = np.asarray(indices[:nnz], dtype=np.int64)
    n_rows_out = n_rows if row_map is None else n_rows_out
    n_cols_out = n_cols if col_map is None else n_cols_out
    ri = i if row_map is None else np.asarray(row_map, dtype=np.int64)[i]
    cj = j if col_map is None else np.asarray(col_map, dtype=np.int64)[j]
    keep = (ri >= 0) & (ri < n_rows_out) & (cj >= 0) & (cj < n_cols_out)
    if entry_keep is not None:
        flag = np.asarray(entry_keep).astype(bool)
        if symmetric_mask:
            where = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(i, j))}
            q = np.array([p if a <= b else where.get((int(b), int(a)), -1) for p, (a, b) in enumerate(zip(i, j))], dtype=np.int64)
            keep &= (q >= 0) & flag[np.maximum(q, 0)]
        else:
            keep &= flag
    if drop_self:
        keep &= i != j
    if drop_below:
        a, b = (np.minimum(i, j), np.maximum(i, j)) if symmetric else (i, j)
        keep &= _hash4(seed, EDGE_DROP_STREAM, a.astype(np.uint64), b.astype(np.uint64)) >= np.uint64(drop_below)
    return keep, ri, cj


def oracle_select(a, **kw):
    """(indptr int64, indices int32, data float32, pos int64) of the selection of the canonical scipy CSR `a`"""
    keep, ri, cj = oracle_keep(a.indptr, a.indices, a.shape[1], **kw)
    n_rows_out = a.shape[0] if kw.get("row_map") is None else kw["n_rows_out"]
    pos = np.nonzero(keep)[0].astype(np.int64)
    pos = pos[np.argsort(ri[pos], kind="stable")]          # monotone maps leave the order as it is
    indptr = np.zeros(n_rows_out + 1, dtype=np.int64)
    np.cumsum(np.bincount(ri[pos], minlength=n_rows_out), out=indptr[1:])
    return indptr, cj[pos].astype(np.int32), np.asarray(a.data, dtype=np.float32)[pos], pos


def oracle_matrix(a, **kw):
    indptr, indices, data, _ = oracle_select(a, **kw)
    n_rows_out = len(indptr) - 1
    n_cols_out = a.shape[1] if kw.get("col_map") is None else kw["n_cols_out"]
    return sp.csr_matrix((data, indices, indptr), shape=(n_rows_out, n_cols_out))


def mask_to_map(mask, keep_ids=False):
    """(int32 old id -> new id or -1, number of new ids): an exclusive scan of the mask, or the identity on the kept ids"""
    mask = np.asarray(mask, dtype=bool)
    ids = np.arange(len(mask)) if keep_ids else np.cumsum(mask) - 1
    return np.where(mask, ids, -1).astype(np.int32), (len(mask) if keep_ids else int(mask.sum()))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_csr(a, b):
    a, b = canonical(a), canonical(b)
    return (a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
            and same_bits(a.data.astype(np.float32), b.data.astype(np.float32)))


def recorded(goldens, key):
    g = goldens.npz("g20_transforms")
    return sp.csr_matrix((g[key + "|data"], g[key + "|indices"], g[key + "|indptr"]), shape=tuple(g[key + "|shape"]))


def g20_graph(goldens, name):
    return recorded(goldens, name) if name == "symdiag48" else canonical(goldens.graph(name).astype(np.float32))


# row lengths around every group size, around the wavefront, and the strided walk
ZOO_LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 129, 300)


def zoo(n_rows=6003, n_cols=7001, seed=5, long_row=5000, mirror=0.0):
    """A canonical CSR (float32) whose row lengths cycle through ZOO_LENGTHS in a shuffled order, with one row of `long_row` entries,
    empty first and last rows, and among the values NaN (with a payload), -0.0, an infinity and a denormal.  6003 rows: no
    multiple of 64, 16 or 4 rows per workgroup.  mirror > 0 (square only): that share of the entries in every third column also gets its mirror, so some
    lower entries have a stored upper partner and some do not; a part of the diagonal is stored."""
    rng = np.random.RandomState(seed)
    lengths = np.array([ZOO_LENGTHS[k % len(ZOO_LENGTHS)] for k in rng.permutation(n_rows)], dtype=np.int64)
    lengths[0] = lengths[-1] = 0
    lengths[n_rows // 3] = long_row
    lengths = np.minimum(lengths, n_cols)
    rows = np.repeat(np.arange(n_rows), lengths)
    cols = np.concatenate([np.sort(rng.choice(n_cols, size=m, replace=False)) for m in lengths if m]) if lengths.sum() else np.zeros(0, int)
    if mirror > 0:
        assert n_rows == n_cols
        pick = rng.rand(len(rows)) < mirror
        pick &= (cols % 3 == 0) & (cols != 0) & (cols != n_rows - 1)     # every third row receives mirrors, the others keep their length;
                                                                         # the first and the last row stay empty
        diag = np.arange(1, n_rows - 1)[rng.rand(n_rows - 2) < 0.3]
        rows, cols = np.concatenate((rows, cols[pick], diag)), np.concatenate((cols, rows[pick], diag))
    a = sp.csr_matrix((np.ones(len(rows), dtype=np.float32), (rows, cols)), shape=(n_rows, n_cols))
    a.sum_duplicates()
    a.sort_indices()
    bits = rng.randint(0, 1 << 32, size=a.nnz, dtype=np.uint64).astype(np.uint32)      # any bit pattern: NaNs with payloads among them
    bits[:4] = (0x7FC01234, 0x80000000, 0x7F800000, 0x00000001)
    a.data = bits.view(np.float32)
    return a

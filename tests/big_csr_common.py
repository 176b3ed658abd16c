"""Shared by test_big_csr_cpu.py and test_gpu_big_csr.py: ONE banded CSR whose every entry is known by formula, at sizes where the
positions into col / val pass 2^31 (tier B) and 2^32 (tier A).  Nothing here needs a GPU: the generator runs on whatever torch device
it is given (the CPU test runs it at a few thousand rows on the CPU), and no HOST array ever has nnz elements.

Structure.  O is a sorted list of distinct integer offsets.  Row i holds the columns i + o for the first w(i) offsets o of O that
land in [0, n_cols): with lo(i) = #{o in O: i + o < 0} and cnt(i) = #{o in O: 0 <= i + o < n_cols},
    len(i) = min(w(i), cnt(i)),    col[rowptr[i] + k] = i + O[lo(i) + k]    (k < len(i)):   sorted and unique -- a canonical row.
Column j is read the other way round: the rows i = j - o, o in O, with 0 <= idx(o) - lo(i) < len(i).  Both are O(|O|) per row on the
host, and the row pointer is one cumulative sum over n_rows numbers.

Widths.  w(i) = `base`, except on residue classes (modulus, residue, width) -- an empty row, a row of one entry, a row long enough
to be cut by the SpMM plan -- and in row 0, which is shorter so that no row boundary is a multiple of `base`.

Values.  "hash": the float32 bits of entry (i, j) are 0x3F000000 | (h(i, j) & 0x7FFFFF), a value in [0.5, 1) (positive: the same
matrix serves the normalisation, whose degrees must stay positive); the symmetric variant hashes (min, max).  "pos": the bits of
entry p are p & 0x7FFFFFFF, for the entry points that only move values."""
import numpy as np

B31, B32 = 1 << 31, 1 << 32
MARGIN = 1 << 20
GIB = 1 << 30
# tier -> (entries the matrix must at least hold, free device memory its cases ask for).  The memory figures are MEASURED: the peak of
# the device memory in use during each case on an MI355X (test_gpu_big_csr.py samples and prints it; the library's own temporaries
# and what torch's allocator still caches from the case before are in it), rounded up.  col + val are 8 bytes an entry: 17.3 GB (B),
# 34.5 GB (A).  An MI355X has 288 GB: on an idle card nothing skips.
TIERS = {"B": (B31 + MARGIN, 130 * GIB),     # beyond a signed 32-bit position; peak 126.2 GiB: the merge with both position outputs
         "A": (B32 + MARGIN, 205 * GIB)}     # beyond an unsigned one, for the entry points without a 2^32 cap; peak 201.7 GiB: the merge
NORM_NEED = 230 * GIB        # whole-matrix normalisation of tier B: sgl_norm_execute(_lr) 178.1 GiB, PreparedAdjacency (directed) 226.3 GiB
INGEST_NEED = 215 * GIB      # sgl_coo_to_csr of 2.16e9 int64 pairs: 210.3 GiB (inputs 43 GB, sort keys / permutation / scan 86 GB, outputs)

P1, P2 = 2147483647, 48271


def hash_np(a, b):
    """h(a, b) for int64 arrays a, b < 2^24: two rounds of a Lehmer-style mix, every intermediate below 2^63 (numpy and torch agree)"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    h = (a * 2654435761 + b * 40503 + 12345) % P1
    return (h * P2 + 11) % P1


def hash_torch(a, b):
    h = (a * 2654435761 + b * 40503 + 12345) % P1
    return (h * P2 + 11) % P1


class BigCSR:
    def __init__(self, n, offsets, base, classes=(), first=None, symmetric=False):
        self.n = int(n)
        self.O = np.asarray(offsets, dtype=np.int64)
        assert np.all(np.diff(self.O) > 0) and self.n < (1 << 24)
        self.base, self.classes, self.first, self.symmetric = int(base), tuple(classes), first, bool(symmetric)
        i = np.arange(self.n, dtype=np.int64)
        self.lo = np.searchsorted(self.O, -i, side="left")
        cnt = np.searchsorted(self.O, self.n - i, side="left") - self.lo
        self.len = np.minimum(self.widths(i), cnt)
        self.rowptr = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(self.len, out=self.rowptr[1:])
        self.nnz = int(self.rowptr[-1])

    # ---- the formulas, host side -------------------------------------------------------------------------------------------
    def widths(self, i):
        i = np.asarray(i, dtype=np.int64)
        w = np.full(i.shape, self.base, dtype=np.int64)
        for m, r, wd in self.classes:
            w[i % m == r] = wd
        if self.first is not None:
            w[i == 0] = self.first
        return w

    def row_class(self, i):
        """"first", "last", the width of the residue class the row is in, or "base" """
        if i == 0 and self.first is not None:
            return "first"
        for m, r, wd in self.classes:
            if i % m == r:
                return wd
        return "last" if i == self.n - 1 else "base"

    def value_bits(self, i, j, p=None, mode="hash"):
        if mode == "pos":
            return (np.asarray(p, dtype=np.int64) & 0x7FFFFFFF).astype(np.uint32)
        i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
        a, b = (np.minimum(i, j), np.maximum(i, j)) if self.symmetric else (i, j)
        return (0x3F000000 | (hash_np(a, b) & 0x7FFFFF)).astype(np.uint32)

    def row(self, i, mode="hash"):
        """(columns int64, values float32, positions int64) of row i"""
        i = int(i)
        k = np.arange(self.len[i], dtype=np.int64)
        c = i + self.O[self.lo[i] + k]
        p = self.rowptr[i] + k
        return c, self.value_bits(np.full(len(k), i), c, p, mode).view(np.float32), p

    def column(self, j, mode="hash"):
        """(rows int64 ascending, values float32, positions int64) of column j"""
        j = int(j)
        idx = np.arange(len(self.O), dtype=np.int64)
        i = j - self.O
        ok = (i >= 0) & (i < self.n)
        i, idx = i[ok], idx[ok]
        k = idx - self.lo[i]
        ok = (k >= 0) & (k < self.len[i])
        i, k = i[ok][::-1], k[ok][::-1]
        p = self.rowptr[i] + k
        return i, self.value_bits(i, np.full(len(i), j), p, mode).view(np.float32), p

    def find(self, i, j):
        """position of (i, j) for arrays of pairs inside the matrix, -1 where it is not stored"""
        i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
        idx = np.minimum(np.searchsorted(self.O, j - i), len(self.O) - 1)
        k = idx - self.lo[i]
        hit = (self.O[idx] == j - i) & (k >= 0) & (k < self.len[i])
        return np.where(hit, self.rowptr[i] + k, -1)

    def entry_at(self, p, mode="hash"):
        """(row, column, value bits) of the entry at position p, from the formulas"""
        i = int(np.searchsorted(self.rowptr, p, side="right") - 1)
        c = i + int(self.O[self.lo[i] + (p - self.rowptr[i])])
        return i, c, int(self.value_bits(i, c, p, mode))

    def sub_matrix(self, rows, mode="hash"):
        """the rows `rows` as a CSR over COMPACT column ids: (indptr, indices int32, values float32, cols) with cols the sorted global
        ids of the columns that occur -- the reference of a sampled-row product needs the rows cols of X and nothing else"""
        got = [self.row(i, mode) for i in rows]
        indptr = np.concatenate(([0], np.cumsum([len(g[0]) for g in got]))).astype(np.int64)
        allc = np.concatenate([g[0] for g in got]) if got else np.zeros(0, np.int64)
        cols, inv = np.unique(allc, return_inverse=True)
        vals = np.concatenate([g[1] for g in got]) if got else np.zeros(0, np.float32)
        return indptr, inv.astype(np.int32), vals.astype(np.float32), cols

    def scipy(self, mode="hash"):
        """the whole matrix (small sizes only)"""
        import scipy.sparse as sp
        assert self.nnz < (1 << 24)
        got = [self.row(i, mode) for i in range(self.n)]
        return sp.csr_matrix((np.concatenate([g[1] for g in got]), np.concatenate([g[0] for g in got]).astype(np.int32), self.rowptr),
                             shape=(self.n, self.n))

    # ---- sampled rows --------------------------------------------------------------------------------------------------------
    def straddler(self, boundary):
        """the row with rowptr[i] < boundary < rowptr[i + 1], or None"""
        i = int(np.searchsorted(self.rowptr, boundary, side="right") - 1)
        return i if i < self.n and self.rowptr[i] < boundary < self.rowptr[i + 1] else None

    def first_of_class(self, after, m, r, count=3):
        i0 = after + ((r - after) % m)
        return [i for i in range(i0, self.n, m)][:count]

    def near_rows(self):
        """64 rows whose entries all lie below 2^30: row 0, rows whose first offsets fall off the left edge, every class"""
        rows = {0, 1, 2, 5, int(-self.O[0]) // 2}
        for m, r, _ in self.classes:
            rows.update(self.first_of_class(1, m, r))
        lim = int(np.searchsorted(self.rowptr, min(1 << 30, self.nnz), side="right") - 2)
        rows.update(np.linspace(3, max(lim, 4), 64).astype(np.int64).tolist())
        rows = sorted(r for r in rows if 0 <= r <= lim)[:64]
        return np.asarray(rows, dtype=np.int64)

    def far_rows(self, boundaries):
        """at least 256 rows fixed by formula: the rows straddling every boundary, and rows that START beyond the LAST one -- the
        first rows after it, the first rows of every class after it, the last rows of the matrix, and an even spread"""
        rows = set()
        start = 0
        for b in boundaries:
            s = self.straddler(b)
            assert s is not None, "no row straddles the boundary"
            rows.add(s)
            start = s + 1
        rows.update(range(start, start + 8))
        for m, r, _ in self.classes:
            rows.update(self.first_of_class(start, m, r))
        rows.update((self.n - 1, self.n - 2, self.n - 3))
        rows.update(np.linspace(start, self.n - 1, 256).astype(np.int64).tolist())
        return np.asarray(sorted(rows), dtype=np.int64)

    # ---- the generator: any torch device, in chunks of positions ------------------------------------------------------------------
    def generate(self, device, mode="hash", chunk=1 << 24, values=True):
        """(rowptr int64 [n + 1], col int32 [nnz], val float32 [nnz]) on `device`; values=False: val is None"""
        import torch
        rp = torch.from_numpy(self.rowptr).to(device)
        lo = torch.from_numpy(self.lo).to(device)
        off = torch.from_numpy(self.O).to(device)
        col = torch.empty(self.nnz, dtype=torch.int32, device=device)
        val = torch.empty(self.nnz, dtype=torch.float32, device=device) if values else None
        bits = val.view(torch.int32) if values else None
        for p0 in range(0, self.nnz, chunk):
            p = torch.arange(p0, min(p0 + chunk, self.nnz), dtype=torch.int64, device=device)
            r = torch.searchsorted(rp, p, right=True) - 1
            c = r + off[lo[r] + (p - rp[r])]
            col[p0:p0 + chunk] = c.to(torch.int32)
            if not values:
                continue
            if mode == "pos":
                bits[p0:p0 + chunk] = (p & 0x7FFFFFFF).to(torch.int32)
            else:
                a, b = (torch.minimum(r, c), torch.maximum(r, c)) if self.symmetric else (r, c)
                bits[p0:p0 + chunk] = (0x3F000000 | (hash_torch(a, b) & 0x7FFFFF)).to(torch.int32)
        return rp, col, val


# ---- the instances ---------------------------------------------------------------------------------------------------------------
def directed_offsets():
    """16384 offsets, -15000 .. 66917, steps of 4 .. 7, not symmetric; 0 is the 3001st, so only rows longer than 3000 entries (and
    the rows near the left edge) store their diagonal"""
    k = np.arange(16384, dtype=np.int64)
    return 5 * k - 15000 + k % 3


def symmetric_offsets():
    """O = -O: +-(7 k + 1 + k % 3), k < 512; no 0, so the normalisation inserts every diagonal entry"""
    k = np.arange(512, dtype=np.int64)
    s = 7 * k + 1 + k % 3
    return np.concatenate((-s[::-1], s))


LONG = 5000                                       # beyond the default long_row_nnz of a matrix of this size (2048): cut into 3 pieces
CLASSES = ((509, 3, 0), (509, 7, 1), (4099, 11, LONG))
SMALL_LONG_ROW_NNZ = 1500                         # the explicit threshold: the same rows, cut into 4 pieces at other places
SIZES = {("directed", "B"): (1 << 21) + 16384, ("directed", "A"): (1 << 22) + 24576, ("symmetric", "B"): (1 << 21) + 12288}
_cache = {}


def directed(n):
    return BigCSR(n, directed_offsets(), 1024, CLASSES, first=700)


def symmetric(n):
    """every landing offset is stored, so (i, j) is stored iff (j, i) is: exactly symmetric, values included; rows near either edge
    are shorter.  It has no width classes -- a width that depends on the row alone breaks the symmetry -- which the directed variant
    carries."""
    return BigCSR(n, symmetric_offsets(), 1024, (), first=None, symmetric=True)


def instance(kind, tier):
    key = (kind, tier)
    if key not in _cache:
        _cache[key] = (directed if kind == "directed" else symmetric)(SIZES[key])
    return _cache[key]


def boundaries(tier):
    return (B31,) if tier == "B" else (B31, B32)


# ---- references evaluated on sampled rows ----------------------------------------------------------------------------------------
def row_degree(g, i):
    """the weighted degree of row i of A + I: the SEQUENTIAL fp64 sum of its values in column order, the diagonal's 1 merged into a
    stored diagonal entry or inserted at its sorted place (what scipy's row sum of A + I adds up)"""
    i = int(i)
    c, v, _ = g.row(i)
    v = v.astype(np.float64)
    k = np.searchsorted(c, i)
    if k < len(c) and c[k] == i:
        v[k] += 1.0
    else:
        v = np.insert(v, k, 1.0)
    return float(np.cumsum(v)[-1])          # cumsum adds one element after the other: the sequential sum


def norm_rows_reference(g, rows, r, alpha=None, deg_cache=None):
    """rows `rows` of adj_to_symmetric_norm(A) = D^(r-1) (A + I)^T D^(-r) [then (1 - alpha) . + alpha I] by its definition
    (sgl/operators/utils.py:76-88 of the reference, as oracle.sym_norm_csr restates it), from the formulas alone:
        A_hat[j, i] = fl(fl(A'[i, j] * deg_j^(r-1)) * deg_i^(-r)),   A' = A + I,   deg = the sequential fp64 row sums of A'
    Output row j = column j of A' = the rows i that store j (the closed-form column) and j itself; the degrees of just those rows
    come from the closed-form rows.  Returns [(columns int32, values float64)] -- float32 rounding is the caller's."""
    deg_cache = {} if deg_cache is None else deg_cache      # shared between the calls for one matrix

    def deg(i):
        i = int(i)
        if i not in deg_cache:
            deg_cache[i] = row_degree(g, i)
        return deg_cache[i]

    def power(d, e):
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.power(np.float64(d), e)
        return 0.0 if np.isinf(x) else x

    out = []
    for j in rows:
        j = int(j)
        i, v, _ = g.column(j)
        v = v.astype(np.float64)
        k = np.searchsorted(i, j)
        if k < len(i) and i[k] == j:
            v[k] += 1.0
        else:
            i, v = np.insert(i, k, j), np.insert(v, k, 1.0)
        lj = power(deg(j), r - 1)
        vals = np.array([(a * lj) * power(deg(q), -r) for q, a in zip(i, v)], dtype=np.float64)
        if alpha is not None:
            vals = (1 - alpha) * vals
            vals[i == j] += alpha
        out.append((i.astype(np.int32), vals))
    return out


def merge_row_reference(g, i, b_cols, b_vals, mode="sum"):
    """row i of the union of the matrix with a canonical B whose row i is (b_cols, b_vals): (cols, value bits, pos_a, pos_b_local)"""
    c, v, p = g.row(i)
    b_cols = np.asarray(b_cols, dtype=np.int64)
    cols = np.union1d(c, b_cols)
    ia, ib = np.searchsorted(c, cols), np.searchsorted(b_cols, cols)
    in_a = (ia < len(c)) & (c[np.minimum(ia, max(len(c) - 1, 0))] == cols) if len(c) else np.zeros(len(cols), bool)
    in_b = (ib < len(b_cols)) & (b_cols[np.minimum(ib, max(len(b_cols) - 1, 0))] == cols) if len(b_cols) else np.zeros(len(cols), bool)
    vals = np.zeros(len(cols), dtype=np.float32)
    vals[in_a] = v[ia[in_a]]
    only_b = in_b & ~in_a
    vals[only_b] = np.asarray(b_vals, dtype=np.float32)[ib[only_b]]
    both = in_a & in_b
    if mode == "sum":
        vals[both] = v[ia[both]] + np.asarray(b_vals, dtype=np.float32)[ib[both]]
    pos_a = np.where(in_a, p[np.minimum(ia, max(len(c) - 1, 0))] if len(c) else -1, -1)
    pos_b = np.where(in_b, ib, -1)
    return cols, vals.view(np.uint32), pos_a, pos_b


def lpa_rows_reference(g, rows, labels, rnd, last):
    """the per-node rule of reorder_common.lpa_round_reference for the rows `rows` alone: each as a block of one row at row0 = i"""
    import reorder_common
    out = np.empty(len(rows), dtype=np.int32)
    for k, i in enumerate(rows):
        c = g.row(i)[0]
        out[k] = reorder_common.lpa_round_reference(np.array([0, len(c)]), c, labels, rnd, last, row0=int(i))[0][0]
    return out


def column_lengths(g, device="cpu"):
    """entries of every column, int64 [n], from lo / len / O alone (never from a generated col array): step k counts the k-th entry
    of every row that has one.  The first `base` steps pass over n numbers, the ones after that over the few long rows.  A torch
    loop: the GPU test runs it on the device, the CPU test against scipy."""
    import torch
    lo = torch.from_numpy(g.lo).to(device)
    ln = torch.from_numpy(g.len).to(device)
    off = torch.from_numpy(g.O).to(device)
    cnt = torch.zeros(g.n, dtype=torch.int64, device=device)
    rows = torch.arange(g.n, dtype=torch.int64, device=device)
    one = torch.ones(g.n, dtype=torch.int64, device=device)
    for k in range(int(g.len.max())):
        rows = rows[ln[rows] > k]
        cnt.index_add_(0, rows + off[lo[rows] + k], one[:rows.numel()])
    return cnt


# ---- which test of test_gpu_big_csr.py runs which entry point (test_big_csr_cpu.py checks this list against include/sgl_hip.h) ------
_SPMM = ("test_spmm_family",)
_NORM = ("test_normalise_whole_matrix_directed", "test_normalise_whole_matrix_symmetric")
_POW = ("test_normalise_with_the_device_pow_directed", "test_normalise_with_the_device_pow_symmetric")
_PREP = ("test_prepared_adjacency_directed", "test_prepared_adjacency_symmetric")
_BLOCK = ("test_normalise_row_blocks",)
COVERED = {
    "sgl_csr_create": _SPMM, "sgl_csr_destroy": _SPMM, "sgl_csr_info": _SPMM, "sgl_csr_set_rowmap": _SPMM,
    "sgl_spmm_f32": _SPMM, "sgl_spmm_multi_f32": _SPMM, "sgl_spmm_chain_f32": _SPMM, "sgl_spmm_axpb_clamp_f32": _SPMM,
    "sgl_spmm_acc_f32": _SPMM, "sgl_spmm_bf16": _SPMM, "sgl_spmm_chain_bf16": _SPMM, "sgl_spmm_acc_bf16": _SPMM,
    "sgl_csr_permute_rows": ("test_permute_rows",), "sgl_reorder_lpa_round": ("test_label_propagation_round",),
    "sgl_norm_prepare": _NORM, "sgl_norm_execute": _POW, "sgl_norm_execute_lr": _NORM, "sgl_norm_degrees": _NORM,
    "sgl_norm_build_symcheck": _PREP, "sgl_norm_block_prepare": _PREP + _BLOCK, "sgl_norm_block_build": _BLOCK,
    "sgl_norm_block_colsum": _BLOCK, "sgl_norm_block_scale": _PREP + _BLOCK, "sgl_norm_block_mix": _BLOCK,
    "sgl_norm_block_diag_positions": _PREP + _BLOCK, "sgl_norm_block_mix_at": _PREP + _BLOCK,
    "sgl_coo_to_csr": ("test_ingest_in_transpose_order_with_pairs_stored_twice", "test_prepared_adjacency_directed"),
    "sgl_csr_find": ("test_find_and_candidates",), "sgl_edge_candidates": ("test_find_and_candidates",),
    "sgl_csr_select_rowptr": ("test_select",), "sgl_csr_select_fill": ("test_select",),
    "sgl_csr_merge_rowptr": ("test_merge",), "sgl_csr_merge_fill": ("test_merge",),
}
EXCLUDED = {
    "sgl_csr_set_values": "stores one pointer in the handle and forms no position; the products that read it are covered",
    "sgl_chain_graph_create": "captures the launches of sgl_spmm_chain_f32 (covered) into a hipGraph: the same kernels and arguments, "
                              "and a capture over a 17 GB matrix would only repeat them",
    "sgl_reorder_community": "the rounds are lpa_round_kernel (covered through sgl_reorder_lpa_round); its result needs 8 dependent "
                             "rounds over ALL rows, so no sampled-row reference exists; its sort is over n nodes, not entries",
    "sgl_edge_loss_grad_f32": "its entry list is the incidence list of a prepared EdgePlan (d_pieces, d_inc_other, d_inc_edge), not a CSR "
                              "of the matrix generated here: positions beyond 2^31 need a plan of more than 2^30 edges of its own "
                              "(DESIGN section 4 lists it as not covered)",
    "sgl_edge_dot_f32": "its entry list indexes rows of dense matrices, not CSR positions: test_gpu_far_offsets.py covers those offsets",
}

"""What the ingest tests share (csrc/sgl_ingest.hip, io.coo_to_csr_device, io.load_custom_homo_raw[_sharded], reorder.permute_csr): a
numpy reference of COO -> canonical CSR, a weight maker under which the order of a sum shows in its bits, and the zoo of edge lists.

The contract: columns sorted inside each row, the entries of one (row, col) pair folded into ONE SEQUENTIAL float32 SUM IN STORAGE
ORDER.  All of it is integers or one chain of IEEE float32 additions, so every comparison made with this module is bit-exact."""
import functools
import zlib

import numpy as np
import scipy.sparse as sp

LONG_RUN = 64          # runs up to here are summed one position at a time over all runs at once, longer ones by np.add.accumulate


def sorted_runs(row, col, n_cols, reverse=False):
    """(order, starts, lengths): the stable sort of the entries by (row, col) and the runs of equal pairs in it.  reverse=True keeps
    the members of a run in REVERSED storage order: what a sort that is not stable may do, and the variant the tests use to show
    that a test would notice."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    key = row * max(int(n_cols), 1) + col
    m = len(key)
    order = (m - 1 - np.argsort(key[::-1], kind="stable")) if reverse else np.argsort(key, kind="stable")
    k = key[order]
    head = np.ones(m, dtype=bool)
    head[1:] = k[1:] != k[:-1]
    starts = np.flatnonzero(head)
    lengths = np.diff(np.append(starts, m))
    return order, starts, lengths


def sequential_sums(v, starts, lengths):
    """the sequential float32 sum v[s] + v[s+1] + ... of every run, left to right"""
    v = np.asarray(v, dtype=np.float32)
    acc = v[starts].copy() if len(starts) else np.zeros(0, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        idx = np.flatnonzero((lengths > 1) & (lengths <= LONG_RUN))
        k = 1
        while idx.size:                                               # position k of every run that has one: float32 + float32
            acc[idx] = acc[idx] + v[starts[idx] + k]
            k += 1
            idx = idx[lengths[idx] > k]
        for i in np.flatnonzero(lengths > LONG_RUN):
            acc[i] = np.add.accumulate(v[starts[i]:starts[i] + lengths[i]], dtype=np.float32)[-1]
    return acc


def coo_to_csr_reference(row, col, val, n_rows, n_cols, reverse=False):
    """(indptr int64 [n_rows + 1], indices int32, values float32, nnz): stable argsort of row * n_cols + col, run heads, every run one
    sequential float32 sum in storage order.  A sum that comes out as zero is still an entry."""
    row, col = np.asarray(row, dtype=np.int64).reshape(-1), np.asarray(col, dtype=np.int64).reshape(-1)
    val = np.asarray(val, dtype=np.float32).reshape(-1)
    order, starts, lengths = sorted_runs(row, col, n_cols, reverse)
    values = sequential_sums(val[order], starts, lengths)
    head = order[starts]
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(row[head], minlength=n_rows), out=indptr[1:])
    return indptr, col[head].astype(np.int32), values, len(starts)


def run_lengths(row, col, n_cols):
    """how many stored entries every output entry was folded from, in output order"""
    return sorted_runs(row, col, n_cols)[2]


def order_sensitive_weights(rng, m):
    """random sign x 2^k, k uniform in [-20, 20], x U(1, 2): three of these rarely add up to the same float32 in two orders"""
    sign = rng.choice(np.array([-1.0, 1.0]), size=m)
    return (sign * np.ldexp(rng.uniform(1.0, 2.0, size=m), rng.integers(-20, 21, size=m))).astype(np.float32)


def scipy_csr(case):
    """what the reference's Edge builds: csr_matrix((w, (row, col)), shape) -- canonical, duplicates summed, zeros kept"""
    a = sp.csr_matrix((case["val"], (case["row"], case["col"])), shape=(case["n_rows"], case["n_cols"]))
    assert a.has_canonical_format and a.dtype == np.float32
    return a


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def same_values(got, want):
    """bit patterns equal; where the reference is a NaN, a NaN (whatever its payload)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return False
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all()) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def changed(a, b):
    """which values differ as bits (two NaNs count as equal)"""
    return (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))


# ---- the zoo -------------------------------------------------------------------------------------------------------------------------
def _case(name, row, col, n_rows, n_cols, rng=None, val=None, long_runs=False, runs_at=None, shuffle=True):
    """long_runs: the case is MEANT to hold pairs stored three times or more.  runs_at: {sorted position: run length} the case is
    built around.  The storage order is shuffled unless the case is about its storage order."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    if rng is not None and shuffle:
        p = rng.permutation(len(row))
        row, col = row[p], col[p]
    if val is None:
        val = order_sensitive_weights(rng, len(row))
        for _ in range(64 if long_runs else 0):                        # a case with one long run: draw until the order shows in it
            fwd, rev = (coo_to_csr_reference(row, col, val, n_rows, n_cols, reverse=r)[2] for r in (False, True))
            if changed(fwd, rev).any():
                break
            val = order_sensitive_weights(rng, len(row))
    return dict(name=name, row=row, col=col, val=np.asarray(val, dtype=np.float32), n_rows=int(n_rows), n_cols=int(n_cols),
                long_runs=bool(long_runs), runs_at=dict(runs_at or {}))


def _cells(cells, n_cols):
    cells = np.asarray(cells, dtype=np.int64)
    return cells // n_cols, cells % n_cols


def _placed_run(name, rng, start, length, n_rows=20, n_cols=50, after=40):
    """`start` single pairs, then one pair stored `length` times -- sorted positions start ... start + length - 1 -- then `after`
    more single pairs; storage order shuffled"""
    cells = np.concatenate((np.arange(start), np.full(length, start), np.arange(start + 1, start + 1 + after)))
    r, c = _cells(cells, n_cols)
    return _case(name, r, c, n_rows, n_cols, rng, long_runs=length >= 3, runs_at={start: length})


def _rng(name, salt=0):
    """one generator per case, seeded by the case's name: adding a case leaves the others as they are"""
    return np.random.default_rng([20261020, zlib.crc32(name.encode()), salt])


ROW_CASE_COLS = (0, 2, 2, 5, 0, 3)        # per occupied row: two pairs stored twice, two once; columns 0 and n_cols - 1 = 5 among them


def _build_zoo():
    zoo = []
    for nnz in (1, 255, 256, 257, 1025):                               # around one and four 256-thread blocks; 8 x 9 cells: many duplicates
        rng = _rng(f"nnz{nnz}")
        zoo.append(_case(f"nnz{nnz}", rng.integers(0, 8, nnz), rng.integers(0, 9, nnz), 8, 9, rng, long_runs=nnz > 1))
    for nnz in (300, 100_000):                                         # one pair: one thread's loop over everything
        name = f"one_key_{nnz}"
        zoo.append(_case(name, np.full(nnz, 1), np.full(nnz, 2), 3, 5, _rng(name), long_runs=True, runs_at={0: nnz}))
    zoo.append(_placed_run("run5_at_254", _rng("run5_at_254"), 254, 5))    # its head in one block, its tail in the next
    zoo.append(_placed_run("run4_at_255", _rng("run4_at_255"), 255, 4))
    zoo.append(_placed_run("run4_at_256", _rng("run4_at_256"), 256, 4))
    # duplicates with the entries of other pairs between them in storage: A B C D A B C D ... (stability keeps every pair's order)
    k = np.tile(np.arange(4), 10)
    zoo.append(_case("interleaved", k // 2, 3 * (k % 2) + 1, 2, 5, _rng("interleaved"), long_runs=True, shuffle=False))
    zoo.append(_case("interleaved_descending", np.tile([2, 1, 0], 7), np.tile([0, 4, 2], 7), 3, 5, _rng("interleaved_descending"),
                     long_runs=True, shuffle=False))
    for n_rows in (1, 2, 3, 4, 5, 1 << 16, (1 << 16) + 1, (1 << 20) + 1):
        # entries in the first and the last row, every row between them empty
        rows = np.unique([0, n_rows - 1])
        name = f"rows{n_rows}_ends"
        zoo.append(_case(name, np.repeat(rows, 6), np.tile(ROW_CASE_COLS, len(rows)), n_rows, 6, _rng(name)))
        if n_rows >= 3:                                                # empty leading and trailing rows (and an interior one from 5)
            rows = np.unique([1, n_rows - 2])
            name = f"rows{n_rows}_inside"
            zoo.append(_case(name, np.repeat(rows, 6), np.tile(ROW_CASE_COLS, len(rows)), n_rows, 6, _rng(name)))
    zoo.append(_case("tall_1_column", [0, 3, 3, 1, 3, 0, 3], [0] * 7, 4, 1, _rng("tall_1_column"), long_runs=True))       # n_rows > n_cols
    zoo.append(_case("wide_7_columns", [0, 2, 2, 0, 2, 1, 2, 0, 0], [0, 6, 6, 6, 0, 3, 6, 6, 6], 3, 7, _rng("wide_7_columns"),
                     long_runs=True))                                                                                      # n_rows < n_cols
    far = (1 << 31) - 2                                                # column ids cost no memory
    cols = np.array([0, far - 1, far - 1, far - 2, 1 << 30, far - 1, 0, 1 << 16, far - 1, far - 2, 1, 0, far - 1, far - 1, 0])
    rows = np.array([0, 0, 4, 4, 2, 0, 4, 2, 0, 4, 2, 4, 0, 4, 4])
    zoo.append(_case("columns_to_2^31-3", rows, cols, 5, far, _rng("columns_to_2^31-3"), long_runs=True))
    one, tiny, inf, nan = np.float32(1), np.float32(2.0 ** -24), np.float32(np.inf), np.float32(np.nan)
    special = [((0, 0), [-0.0]),                                       # a stored -0.0 alone keeps its sign
               ((0, 1), [3.5, -3.5]),                                  # cancels to +0.0: still an entry
               ((0, 2), [1.5, 2.5, -4.0]),                             # three that cancel exactly
               ((1, 0), [inf, -inf]),                                  # NaN
               ((1, 1), [1.0, nan, 2.0]),                              # a NaN in the middle of a run
               ((1, 2), [-0.0, -0.0]),
               ((2, 0), [one, tiny, tiny]),                            # 1 in this order, 1 + 2^-23 in the other
               ((2, 2), [inf])]
    r, c, v = [], [], []
    for pos in range(3):                                               # member `pos` of every run: other pairs lie between a run's members
        for (i, j), members in special:
            if pos < len(members):
                r.append(i), c.append(j), v.append(members[pos])
    zoo.append(_case("special_values", r, c, 4, 3, val=np.array(v, dtype=np.float32), long_runs=True))
    zoo.append(_case("empty_0_rows", [], [], 0, 0, val=[]))
    zoo.append(_case("empty_5_rows", [], [], 5, 5, val=[]))
    # square, one heavy row (nnz-balanced cuts leave ranks without rows), every pair stored about 12 times all over the list: the
    # members of a run lie in different chunks of the sharded reader
    n = 23
    rng = _rng("sharded_square")
    heavy = 3 * n + rng.integers(0, n, 16)[rng.integers(0, 16, 200)]
    light = rng.integers(0, n * n, 4)[rng.integers(0, 4, 40)]
    r, c = _cells(np.concatenate((heavy, light)), n)
    zoo.append(_case("sharded_square", r, c, n, n, rng, long_runs=True))
    assert len({z["name"] for z in zoo}) == len(zoo)
    return zoo


ZOO = _build_zoo()
ZOO_NAMES = [z["name"] for z in ZOO]
BY_NAME = {z["name"]: z for z in ZOO}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(indptr, indices, values, nnz, run lengths) of a zoo case: computed once, shared, never written to"""
    z = BY_NAME[name]
    out = coo_to_csr_reference(z["row"], z["col"], z["val"], z["n_rows"], z["n_cols"]) + (run_lengths(z["row"], z["col"], z["n_cols"]),)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def error_list(seed=3, m=600, n_rows=40, n_cols=50):
    """a valid list of m entries over a rectangular shape, for the error contract"""
    rng = np.random.default_rng(seed)
    return _case("error_list", rng.integers(0, n_rows, m), rng.integers(0, n_cols, m), n_rows, n_cols, rng)


def bad_indices(n_rows, n_cols):
    """(name, array, value): every way one index can lie outside; the last two have low 32 bits that look valid"""
    return [("row = -1", "row", -1), ("row = n_rows", "row", n_rows), ("col = -1", "col", -1), ("col = n_cols", "col", n_cols),
            ("row = 2^32 + 3", "row", (1 << 32) + 3), ("col = 2^32 + 1", "col", (1 << 32) + 1)]

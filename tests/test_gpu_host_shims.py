"""The host data path of sgl_amd/csrc/sgl_shims.hip on a real MI355X: the reference-signature shims FloatCSRMulDense[OMP] with their
row pieces, staged multi-chunk copies and cached adjacency, and sgl_download.  Run with `-m gpu`.

The reference everywhere is oracle.oracle_spmm (the C restatement of the reference's fmaf chain; `out=` for its accumulate
semantics).  The shims run strict order, so every comparison is exact: np.array_equal, and by bit pattern where -0.0 matters
(a NaN must be a NaN at the same place; its payload is the adder's business).  The raw symbols are called through ctypes as a
caller written against the reference's libmatmul.so would call them.

Every array that is handed to a shim is kept alive for the life of the module: the cache is keyed on the ADDRESSES of indptr /
indices next to the contents, and a freed array's address can be handed out again for an array of equal content."""
import ctypes
import threading

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import oracle
from inputs import hash_matrix
from sgl_amd import _lib

pytestmark = pytest.mark.gpu

K_CHUNK = 16 << 20            # kChunk of sgl_shims.hip: the staging granularity
PIECES = 8                    # kPieces, requested from nnz >= 2^22
KEEP = []                     # see the module docstring


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def keep(*arrays):
    KEEP.extend(arrays)
    return arrays if len(arrays) > 1 else arrays[0]


def stats():
    h, m = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().sgl_shim_cache_stats(ctypes.byref(h), ctypes.byref(m)))
    return np.array([h.value, m.value])


def overwrite(csr, x, answer=None):
    """FloatCSRMulDense as cudamatmul.c declares it; -> (return code, answer)"""
    ptr, col, val = csr
    n, d = x.shape
    answer = np.full((n, d), np.nan, np.float32) if answer is None else answer
    rc = _lib.lib().FloatCSRMulDense(p(answer), int(ptr[n]), p(val), p(col), p(ptr), p(x), n, d)
    return rc, answer


def accumulate(csr, x, answer):
    """FloatCSRMulDenseOMP as matmul.h declares it (no return value: the error text is the channel)"""
    ptr, col, val = csr
    n, d = x.shape
    _lib.lib().FloatCSRMulDenseOMP(p(answer), p(val), p(col), p(ptr), p(x), n, d)
    assert _lib.last_error() == "", _lib.last_error()
    return answer


def same_bits(got, want):
    """bit for bit, -0.0 and +0.0 apart; NaN exactly where the reference has NaN"""
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def small_csr(goldens, name):
    """a golden graph, normalised, as the int32 / float32 arrays the reference's wrapper hands over"""
    g = goldens.graph(name)
    n = g.shape[0]
    ptr, col, val = oracle.sym_norm_csr(g.indptr, g.indices, g.data, n, 0.5, None)
    return keep(np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(col, np.int32), np.ascontiguousarray(val, np.float32))


# ---- eight pieces, several chunks -----------------------------------------------------------------------------------------------------
BIG_N, BIG_D = 700_001, 16


def big_csr(n, last_rows_empty):
    """canonical CSR by formula: hashed base degrees 0 .. 10 (empty rows included) with columns start + j * step in increasing order,
    one row that holds EVERY column at 0.51 n, one more as the last row -- or, with last_rows_empty, as row n - 2 with rows 0 and
    n - 1 empty.  Values: the 24-bit dyadic hash of tests/golden/inputs.py."""
    r = np.arange(n, dtype=np.uint64)
    h = r * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    deg = (h % np.uint64(11)).astype(np.int64)
    full = np.zeros(n, bool)
    full[[int(0.51 * n), n - 2 if last_rows_empty else n - 1]] = True
    if last_rows_empty:
        deg[[0, n - 1]] = 0
    deg[full] = n
    ptr = np.concatenate([[0], np.cumsum(deg)])
    nnz = int(ptr[-1])
    step = n // 11 + 1
    start = ((h >> np.uint64(8)) % np.uint64(n - 10 * step)).astype(np.int64)
    rows = np.repeat(np.arange(n), deg)
    j = np.arange(nnz) - ptr[rows]
    col = np.where(full[rows], j, start[rows] + j * step)
    val = hash_matrix(nnz, 1, seed=77).reshape(-1)
    return ptr.astype(np.int32), col.astype(np.int32), val, np.flatnonzero(full)


def piece_boundaries(ptr, n, nnz):
    """build_pieces' rule restated: the p-th of 8 targets nnz * p / 8 goes to lower_bound(row pointers), a boundary that repeats the
    previous one is dropped, one that is not below n is dropped; -> (boundaries, targets de-duplicated, targets dropped at the end)"""
    want = PIECES if nnz >= 1 << 22 else 1
    rows, repeated, beyond = [0], [], []
    for q in range(1, want):
        target = nnz * q // want
        r = min(max(int(np.searchsorted(ptr, target, side="left")), rows[-1]), n)
        if r > rows[-1] and r < n:
            rows.append(r)
        elif r >= n:
            beyond.append(target)
        else:
            repeated.append(target)
    return rows + [n], repeated, beyond


class Big:
    def __init__(self, last_rows_empty):
        n, d = BIG_N, BIG_D
        self.ptr, self.col, self.val, self.full = keep(*big_csr(n, last_rows_empty))
        self.csr = (self.ptr, self.col, self.val)
        self.n, self.nnz = n, int(self.ptr[n])
        self.x = keep(hash_matrix(n, d, seed=5))
        self.x2 = keep(hash_matrix(n, d, seed=6))
        self.ref = oracle.oracle_spmm(self.ptr, self.col, self.val, self.x)
        self.ref2 = oracle.oracle_spmm(self.ptr, self.col, self.val, self.x2)
        self.empty = np.flatnonzero(np.diff(self.ptr) == 0)
        for a in (self.ptr, self.col, self.val, self.x, self.x2, self.ref, self.ref2):
            a.setflags(write=False)                                    # shared between the tests: nobody edits them

    def check_shape(self, last_rows_empty):
        """the preconditions of the edges this matrix exists for, so that no test passes by missing them"""
        n, nnz, ptr = self.n, self.nnz, self.ptr
        assert nnz >= (1 << 22) and nnz % 4 and (np.diff(ptr) >= 0).all() and self.col.min() == 0 and self.col.max() == n - 1
        rows = np.repeat(np.arange(n), np.diff(ptr))
        assert (np.diff(self.col.astype(np.int64)) > 0)[np.diff(rows) == 0].all()                     # canonical: sorted, no duplicates
        assert K_CHUNK < nnz * 4 < 2 * K_CHUNK and (nnz * 4) % K_CHUNK                                # indices, values: 2 chunks, ragged
        assert 2 * K_CHUNK < n * BIG_D * 4 < 3 * K_CHUNK and (n * BIG_D * 4) % K_CHUNK                # X, answer: 3 chunks, ragged
        assert len(self.empty) > n // 20 and (np.diff(ptr)[self.full] == n).all() and len(self.full) == 2
        bounds, repeated, beyond = piece_boundaries(ptr, n, nnz)
        mid, last = self.full
        assert n > nnz // PIECES                                                                      # a full row is longer than a piece
        inside_mid = [t for t in (nnz * q // PIECES for q in range(1, PIECES)) if ptr[mid] < t <= ptr[mid + 1]]
        assert len(inside_mid) == 2 and repeated == inside_mid[1:] and mid + 1 in bounds              # two targets in one row: one boundary
        assert 3 <= len(bounds) - 1 < PIECES and (np.diff(bounds) > 0).all()
        if last_rows_empty:
            assert ptr[1] == 0 and ptr[n - 1] == ptr[n] and last == n - 2 and not beyond
            assert bounds[-2] == n - 1                                                                # the last piece is ONE EMPTY ROW
        else:
            assert last == n - 1 and len(beyond) == 1 and ptr[n - 1] < beyond[0] <= ptr[n]            # a target inside the last row: r = n, dropped
        return bounds


@pytest.fixture(scope="module")
def big():
    b = Big(False)
    b.check_shape(False)
    return b


@pytest.fixture(scope="module")
def big_ends_empty():
    b = Big(True)
    b.check_shape(True)
    return b


def answer_with_specials(n, d, rows):
    """hashed values with one NaN row, one +inf and one -inf, in rows that hold entries"""
    a = hash_matrix(n, d, seed=9)
    a[rows[0], :] = np.nan
    a[rows[1], 3 % d] = np.inf
    a[rows[2], 5 % d] = -np.inf
    return a


def test_big_overwrite_and_accumulate_in_every_piece(cuda, big):
    n, d = big.n, BIG_D
    s0 = stats()
    rc, y = overwrite(big.csr, big.x)                                       # into NaN: every element is overwritten
    assert rc == 0 and np.array_equal(stats() - s0, [0, 1])
    assert same_bits(y, big.ref) and not y[big.empty].view(np.uint32).any()      # empty rows: +0.0
    y0 = accumulate(big.csr, big.x, np.zeros((n, d), np.float32))           # all zeros: the shim skips the answer's upload
    assert same_bits(y0, big.ref)
    neg = np.full((n, d), -0.0, np.float32)                                 # all -0.0: NOT zero for the scan; empty rows keep -0.0
    want = oracle.oracle_spmm(*big.csr, big.x, out=neg.copy())
    assert (want[big.empty].view(np.uint32) == 0x80000000).all()
    assert same_bits(accumulate(big.csr, big.x, neg), want)
    busy = np.flatnonzero(np.diff(big.ptr) > 0)
    special = answer_with_specials(n, d, [busy[7], busy[len(busy) // 2], int(big.full[1])])
    want = oracle.oracle_spmm(*big.csr, big.x, out=special.copy())
    assert np.isnan(want[busy[7]]).all() and np.isinf(want).sum() == 2
    assert same_bits(accumulate(big.csr, big.x, special), want)
    # the same arrays again: a hit; a new X: still a hit; both exact
    s1 = stats()
    assert np.array_equal(s1 - s0, [3, 1])
    rc, y = overwrite(big.csr, big.x)
    rc2, y2 = overwrite(big.csr, big.x2)
    assert rc == 0 and rc2 == 0 and np.array_equal(stats() - s1, [2, 0])
    assert same_bits(y, big.ref) and same_bits(y2, big.ref2)


def test_big_with_empty_first_and_last_rows(cuda, big_ends_empty):
    b = big_ends_empty
    s0 = stats()
    rc, y = overwrite(b.csr, b.x)
    assert rc == 0 and same_bits(y, b.ref) and not y[[0, b.n - 1]].view(np.uint32).any()
    busy = np.flatnonzero(np.diff(b.ptr) > 0)
    special = answer_with_specials(b.n, BIG_D, [busy[3], int(b.full[0]), busy[-2]])
    special[[0, b.n - 1]] = -0.0
    want = oracle.oracle_spmm(*b.csr, b.x2, out=special.copy())
    got = accumulate(b.csr, b.x2, special)
    assert same_bits(got, want) and (got[[0, b.n - 1]].view(np.uint32) == 0x80000000).all()
    assert np.array_equal(stats() - s0, [1, 1])


# ---- cache history --------------------------------------------------------------------------------------------------------------------
def test_cache_history(goldens, cuda, big):
    """one sequence of calls, the exact hit / miss delta and the exact product after each"""
    from sgl_amd.operators.utils import csr_sparse_dense_matmul
    sym, dir40, pl = (small_csr(goldens, g) for g in ("sym64", "dir40", "pl2000"))

    def product(csr, d, seed, want_delta, note):
        n = len(csr[0]) - 1
        x = keep(hash_matrix(n, d, seed=seed))
        s = stats()
        rc, y = overwrite(csr, x)
        assert rc == 0 and same_bits(y, oracle.oracle_spmm(*csr, x)), note
        assert np.array_equal(stats() - s, want_delta), (note, stats() - s)

    miss, hit = [0, 1], [1, 0]
    product(sym, 5, 1, miss, "a small graph first: whatever was cached before this test is gone")
    s = stats()
    rc, y = overwrite(big.csr, big.x)
    assert rc == 0 and same_bits(y, big.ref) and np.array_equal(stats() - s, miss)
    product(dir40, 9, 2, miss, "big -> small: the device buffers keep the larger capacity")
    product(dir40, 9, 3, hit, "small again")
    s = stats()
    rc, y = overwrite(big.csr, big.x2)
    assert rc == 0 and same_bits(y, big.ref2) and np.array_equal(stats() - s, miss)                  # big again, into the kept buffers
    product(pl, 100, 4, miss, "pl2000")
    product(pl, 8, 5, hit, "d 100 -> 8 on a hit")
    product(pl, 147, 6, hit, "d 8 -> 147 on a hit: the dense buffers grow, the adjacency stays")

    ptr, col, val = pl
    r = int(np.flatnonzero((np.diff(ptr)[:-1] > 1) & (np.diff(ptr)[1:] > 0))[10])
    ptr[r + 1] -= 1                                                           # row r's last entry now opens row r + 1, in place
    product(pl, 100, 7, miss, "one entry moved between neighbouring rows of indptr")
    product(pl, 100, 8, hit, "and kept")
    col[ptr[r] + 0] = (col[ptr[r]] + 1000) % 2000
    product(pl, 100, 9, miss, "one column index edited in place")
    val[len(val) // 2 + 3] *= 3.0
    product(pl, 100, 10, miss, "one value edited in place")
    assert val[1] != 0 and val[9] != 0
    val[[1, 9]] *= -1                                                         # float32 words 0 and 4: one lane of the hash, both sign bits
    product(pl, 100, 11, miss, "two same-lane values negated in place")
    product(pl, 100, 12, hit, "and kept")
    assert val[8] != 0
    val[[1, 8, 9]] *= -1                                                      # word 0's upper half and BOTH halves of word 4, the lane's next
    product(pl, 100, 16, miss, "three same-lane values negated in place: a sign flip and both signs of the lane's next word")
    product(pl, 100, 17, hit, "and kept")
    twin = keep(ptr.copy(), col.copy(), val.copy())
    product(twin, 100, 13, miss, "equal content at new addresses: a miss by design")
    product(pl, 100, 14, miss, "and the first set of arrays again")

    # the reference's wrapper: float64 data, converted to a NEW float32 array on every call (only indptr / indices keep their addresses)
    g = goldens.graph("pl2000")
    n = g.shape[0]
    gp, gc, gv = oracle.sym_norm_csr(g.indptr, g.indices, g.data, n, 0.5, None)
    adj = sp.csr_matrix((gv.astype(np.float64), gc.astype(np.int32), gp.astype(np.int32)), shape=(n, n))
    keep(adj.indptr, adj.indices, adj)
    x = keep(hash_matrix(n, 37, seed=15))
    # after astype(float32), (1, 9) and (4001, 4009) are upper halves of two words of ONE lane and (1, 8, 9) adds the lower half of
    # the second: these are the sharp cases, which a hash that lets same-lane sign flips cancel serves from the cache.  (1, 5) is
    # words 0 and 2, two lanes: any order-sensitive hash tells it apart, it is here as one more ordinary edit.
    for pair in ((1, 9), (1, 5), (4001, 4009), (1, 8, 9)):
        s = stats()
        assert np.array_equal(csr_sparse_dense_matmul(adj, x), oracle.oracle_spmm(gp, gc, adj.data.astype(np.float32), x))
        assert (stats() - s).sum() == 1
        assert (adj.data[list(pair)] != 0).all()
        adj.data[list(pair)] *= -1
        s = stats()
        assert np.array_equal(csr_sparse_dense_matmul(adj, x), oracle.oracle_spmm(gp, gc, adj.data.astype(np.float32), x)), pair
        assert np.array_equal(stats() - s, miss), pair


# ---- degenerate and refused calls -----------------------------------------------------------------------------------------------------
def test_degenerate_calls_touch_nothing(goldens, cuda):
    lib = _lib.lib()
    ptr, col, val = small_csr(goldens, "dir40")
    n = len(ptr) - 1
    x = keep(hash_matrix(n, 6, seed=1))
    guard = np.full((n, 6), 7.5, np.float32)
    s = stats()
    for rows, cols in ((0, 6), (n, 0), (0, 0)):
        assert lib.FloatCSRMulDense(p(guard), int(ptr[rows]), p(val), p(col), p(ptr), p(x), rows, cols) == 0 and _lib.last_error() == ""
        lib.FloatCSRMulDenseOMP(p(guard), p(val), p(col), p(ptr), p(x), rows, cols)
        assert _lib.last_error() == ""
    assert (guard == 7.5).all() and np.array_equal(stats() - s, [0, 0])
    # no entries at all, data and indices NULL: answer += 0 leaves the answer, answer = 0 writes zeros
    none = keep(np.zeros(n + 1, np.int32))
    held = hash_matrix(n, 6, seed=2)
    held[3, 2] = -0.0
    got = held.copy()
    lib.FloatCSRMulDenseOMP(p(got), None, None, p(none), p(x), n, 6)
    assert _lib.last_error() == "" and same_bits(got, held)
    assert lib.FloatCSRMulDense(p(got), 0, None, None, p(none), p(x), n, 6) == 0 and _lib.last_error() == ""
    assert not got.view(np.uint32).any()
    rc, y = overwrite((ptr, col, val), x)                                     # and a real matrix right after the handle over no entries
    assert rc == 0 and same_bits(y, oracle.oracle_spmm(ptr, col, val, x))


def test_refused_calls_say_why_and_write_nothing(goldens, cuda):
    lib = _lib.lib()
    ptr, col, val = small_csr(goldens, "sym64")
    n = len(ptr) - 1
    nnz = int(ptr[n])
    x = keep(hash_matrix(n, 5, seed=3))
    want = oracle.oracle_spmm(ptr, col, val, x)
    shifted = keep(ptr + 1)                                                   # indptr[0] = 1, indptr[n] = nnz + 1
    longer_val, longer_col = keep(np.append(val, np.float32(1)), np.append(col, np.int32(0)))
    guard = np.full((n, 5), -3.25, np.float32)
    for args, word in (((p(guard), nnz + 1, p(val), p(col), p(ptr), p(x), n, 5), "data_nnz"),
                       ((p(guard), nnz - 1, p(val), p(col), p(ptr), p(x), n, 5), "data_nnz"),
                       ((p(guard), nnz + 1, p(longer_val), p(longer_col), p(shifted), p(x), n, 5), "bad indptr"),
                       ((p(guard), nnz, p(val), p(col), p(ptr), p(x), -1, 5), "negative"),
                       ((p(guard), nnz, p(val), p(col), p(ptr), p(x), n, -1), "negative")):
        s = stats()
        assert lib.FloatCSRMulDense(*args) == 1, word
        assert word in _lib.last_error(), (word, _lib.last_error())
        assert (guard == -3.25).all() and np.array_equal(stats() - s, [0, 0]), word
        rc, y = overwrite((ptr, col, val), x)                                 # the next valid call is unaffected
        assert rc == 0 and _lib.last_error() == "" and same_bits(y, want), word
    # the symbol without a return value reports through the error text alone
    lib.FloatCSRMulDenseOMP(p(guard), p(longer_val), p(longer_col), p(shifted), p(x), n, 5)
    assert "bad indptr" in _lib.last_error() and (guard == -3.25).all()
    lib.FloatCSRMulDenseOMP(p(guard), p(val), p(col), p(ptr), p(x), -1, 5)
    assert "negative" in _lib.last_error() and (guard == -3.25).all()
    assert same_bits(accumulate((ptr, col, val), x, np.zeros((n, 5), np.float32)), want)


# ---- two host threads -----------------------------------------------------------------------------------------------------------------
def test_two_host_threads_share_the_shim(goldens, cuda):
    """ctypes releases the GIL and the shim serialises on its mutex: two threads, each with its own matrix, meet at a barrier before
    every call, so the two calls of a round are in flight together and the cached adjacency changes hands between them"""
    jobs = []
    for name, d in (("pl2000", 24), ("dir40", 7)):
        csr = small_csr(goldens, name)
        xs = [keep(hash_matrix(len(csr[0]) - 1, d, seed=20 + k)) for k in range(4)]
        jobs.append((csr, xs, [oracle.oracle_spmm(*csr, x) for x in xs]))
    barrier = threading.Barrier(2, timeout=60)
    results, errors = [[], []], []

    def work(t):
        try:
            torch.cuda.set_device(0)
            csr, xs, _ = jobs[t]
            for x in xs:
                barrier.wait()
                results[t].append(overwrite(csr, x))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
            barrier.abort()

    s = stats()
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not errors and not any(th.is_alive() for th in threads), errors
    assert (stats() - s).sum() == 8
    for t in range(2):
        assert len(results[t]) == 4
        for (rc, y), want in zip(results[t], jobs[t][2]):
            assert rc == 0 and same_bits(y, want), t


# ---- sgl_download ---------------------------------------------------------------------------------------------------------------------
ODD = 0x9E3779B97F4A7C15


def formula_bytes(nbytes):
    """the bytes of word[j] = j * ODD (mod 2^64), j = 0, 1, ...: what the device fills its source with"""
    words = np.arange((nbytes + 7) // 8, dtype=np.uint64) * np.uint64(ODD)
    return words.view(np.uint8)[:nbytes]


@pytest.mark.parametrize("nbytes", [0, 1, 3, K_CHUNK - 4, K_CHUNK, K_CHUNK + 4, 33 * K_CHUNK + 12])
def test_download_of_every_chunk_count(cuda, nbytes):
    """device -> pageable host through the pinned staging team.  The team has at most 32 members, so 33 chunks + 12 bytes is the
    smallest transfer at which a member must refill its pinned buffer whatever the team size.  Source and destination are both only
    1-byte aligned, each between guards; the source is filled on the device by formula and never travels any other way."""
    n_words = (nbytes + 7) // 8
    signed_odd = ODD - (1 << 64)                                              # the same multiplier as torch's wrapping int64 sees it
    src_room = torch.full((nbytes + 17,), 0x5A, dtype=torch.uint8, device=cuda)
    if nbytes:
        words = torch.arange(n_words, dtype=torch.int64, device=cuda) * signed_odd
        src_room[1:1 + nbytes] = words.view(torch.uint8)[:nbytes]
        del words
    dst_room = np.full(nbytes + 65, 0xA5, np.uint8)
    rc = _lib.lib().sgl_download(ctypes.c_void_p(dst_room.ctypes.data + 1), ctypes.c_void_p(src_room.data_ptr() + 1), nbytes,
                                 _lib.current_stream_ptr())
    assert rc == 0, _lib.last_error()
    assert dst_room[0] == 0xA5 and (dst_room[1 + nbytes:] == 0xA5).all()
    assert np.array_equal(dst_room[1:1 + nbytes], formula_bytes(nbytes))
    assert int(src_room[0]) == 0x5A and bool((src_room[1 + nbytes:] == 0x5A).all())


# ---- hop cache end to end -------------------------------------------------------------------------------------------------------------
def test_hop_cache_tells_paired_negations_apart(goldens, cuda, tmp_path):
    """features x and x' = x with two same-lane entries negated (x'' : three, a sign flip and both signs of the lane's next word) are
    other keys of the on-disk hop cache: the call is a miss and returns the hops of x', not the stored hops of x"""
    from sgl_amd.operators.graph_op import LaplacianGraphOp
    g = goldens.graph("pl2000")
    x = hash_matrix(2000, 36, seed=3)
    x2 = x.copy()
    assert x2[0, 1] != 0 and x2[0, 9] != 0
    x2[0, [1, 9]] *= -1                                                       # flat float32 indices 1 and 9: words 0 and 4, one lane
    first = LaplacianGraphOp(prop_steps=2, hop_cache_dir=tmp_path)
    first.propagate(g, x)
    assert (first._hop_cache.hits, first._hop_cache.misses) == (0, 1)
    second = LaplacianGraphOp(prop_steps=2, hop_cache_dir=tmp_path)
    got = second.propagate(g, x2)
    assert (second._hop_cache.hits, second._hop_cache.misses) == (0, 1)
    want = LaplacianGraphOp(prop_steps=2).propagate(g, x2)
    assert len(got) == 3 and all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(got, want))
    assert not torch.equal(got[1].cpu(), first.propagate(g, x)[1].cpu())
    assert (first._hop_cache.hits, first._hop_cache.misses) == (1, 1)
    x3 = x.copy()
    assert x3[0, 8] != 0
    x3[0, [1, 8, 9]] *= -1                                                    # flat indices 1, 8, 9: word 0's upper half, both halves of word 4
    third = LaplacianGraphOp(prop_steps=2, hop_cache_dir=tmp_path)
    got3 = third.propagate(g, x3)
    assert (third._hop_cache.hits, third._hop_cache.misses) == (0, 1)
    want3 = LaplacianGraphOp(prop_steps=2).propagate(g, x3)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(got3, want3)) and not torch.equal(got3[1].cpu(), got[1].cpu())

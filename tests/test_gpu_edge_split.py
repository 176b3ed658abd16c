"""The edge split on a real MI355X (csrc/sgl_edge_split.hip, device.csr_find / edge_candidates, tricks.has_edges / mask_test_edges):
run with `-m gpu`.

Everything here is integers, so every comparison is exact: sgl_csr_find against a dictionary of the stored pairs, sgl_edge_candidates
against the numpy mirror of the stream, mask_test_edges against the sequential oracle of edge_split_common (the reference's loop over
that stream) -- all seven outputs, order included."""
from ctypes import c_void_p

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import edge_split_common as common
from inputs import hash_positive
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.io import DeviceAdjacency
from sgl_amd.tricks import EdgeSplit, has_edges, mask_test_edges, nafs_link_prediction

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A
N_GUARD = 4


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def guarded(n_words, cuda, odd=False):
    """(whole buffer, data pointer of its n_words payload): N_GUARD guard words on either side; odd: the payload starts on an odd
    multiple of 8 bytes (torch allocations are aligned far beyond 16)"""
    lead = N_GUARD + (1 if odd else 0)
    buf = torch.full((lead + n_words + N_GUARD,), GUARD, dtype=torch.int64, device=cuda)
    assert (buf.data_ptr() + 8 * lead) % 16 == (8 if odd else 0)
    return buf, lead


def guards_intact(buf, lead, n_words):
    return bool((buf[:lead] == GUARD).all()) and bool((buf[lead + n_words:] == GUARD).all())


# ---- 1. csr_find --------------------------------------------------------------------------------------------------------------------------
N_ROWS, N_COLS = 6000, 10002


def find_matrix():
    """row 0: the 5000 even columns 2 .. 10000 (13 bisection steps, an absent value between any two stored ones); row 1 empty; row 2 of
    length 1; row 3 empty; then short random rows, some empty; the last row ends on the last column"""
    rng = np.random.default_rng(6000)
    rows = [np.arange(2, 10001, 2), np.array([], np.int64), np.array([7]), np.array([], np.int64)]
    for r in range(4, N_ROWS):
        k = int(rng.integers(0, 10))
        rows.append(np.sort(rng.choice(N_COLS, k, replace=False)))
    rows[-1] = np.array([0, 17, N_COLS - 1])
    indptr = np.zeros(N_ROWS + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    indices = np.concatenate(rows).astype(np.int32)
    return sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(N_ROWS, N_COLS))


def find_queries(a):
    rng = np.random.default_rng(6001)
    coo = a.tocoo()
    stored = np.stack((coo.row, coo.col), 1).astype(np.int64)                    # first and last elements of every row among them
    cols0 = np.concatenate((np.arange(1, 10001, 2), [0, 1, 10001]))              # the odd columns, below the first, above the last
    row0 = np.stack((np.zeros(len(cols0), np.int64), cols0), 1)
    edge = np.array([[0, 0], [0, 1], [0, 10001], [2, 6], [2, 7], [2, 8], [2, 0], [2, N_COLS - 1], [1, 0], [1, 5], [3, N_COLS - 1],
                     [N_ROWS - 1, N_COLS - 1], [N_ROWS - 1, N_COLS - 2], [N_ROWS - 1, 0], [N_ROWS - 1, 1]], np.int64)
    near = stored[rng.choice(len(stored), 3000, replace=False)] + np.array([0, 1])   # the column after a stored one
    near = near[near[:, 1] < N_COLS]
    rand = np.stack((rng.integers(0, N_ROWS, 4000), rng.integers(0, N_COLS, 4000)), 1)
    neg = stored[rng.choice(len(stored), 500, replace=False)] - np.array([N_ROWS, N_COLS])          # both negative
    neg_u = stored[rng.choice(len(stored), 500, replace=False)] - np.array([N_ROWS, 0])
    neg_v = rand[:500] - np.array([0, N_COLS])
    out = np.array([[N_ROWS, 0], [0, N_COLS], [-N_ROWS - 1, 5], [5, -N_COLS - 1], [2 ** 40, 1], [1, -2 ** 62], [0, 2 ** 31 + 2],
                    [0, 2 ** 32 + 2], [-2 ** 63, 2], [2 ** 63 - 1, 2 ** 63 - 1], [N_ROWS, N_COLS]], np.int64)
    q = np.concatenate((stored, row0, edge, near, rand, neg, neg_u, neg_v, out))
    return q[rng.permutation(len(q))]


def find_reference(a, q):
    where = {}
    for r in range(a.shape[0]):
        for p in range(a.indptr[r], a.indptr[r + 1]):
            where[(r, int(a.indices[p]))] = p
    want = np.empty(len(q), np.int64)
    for k, (u, v) in enumerate(q.tolist()):
        u = u + N_ROWS if u < 0 else u
        v = v + N_COLS if v < 0 else v
        want[k] = where.get((u, v), -1)
    return want


def test_csr_find_against_numpy(cuda):
    a = find_matrix()
    q = find_queries(a)
    want = find_reference(a, q)
    assert (want >= 0).sum() > 30000 and (want < 0).sum() > 9000
    adj = DeviceAdjacency.from_scipy(a, device=cuda)
    dq = torch.from_numpy(q).to(cuda)
    got = dev.csr_find(adj, dq)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(has_edges(adj, dq).cpu().numpy(), want >= 0)
    # the raw entry: guard words around d_pos, both alignments of the list, the short lengths
    for n_q in (1, 63, 64, 65, 1000, len(q)):
        for odd in (False, True):
            ebuf, elead = guarded(2 * n_q, cuda, odd)
            ebuf[elead:elead + 2 * n_q] = dq[:n_q].reshape(-1)
            pbuf, plead = guarded(n_q, cuda)
            dev._call(cuda, "sgl_csr_find", _lib.ptr(adj.rowptr), _lib.ptr(adj.col), N_ROWS, N_COLS, c_void_p(ebuf.data_ptr() + 8 * elead),
                      n_q, c_void_p(pbuf.data_ptr() + 8 * plead))
            torch.cuda.synchronize()
            assert np.array_equal(pbuf[plead:plead + n_q].cpu().numpy(), want[:n_q]), (n_q, odd)
            assert guards_intact(pbuf, plead, n_q) and guards_intact(ebuf, elead, 2 * n_q), (n_q, odd)
    # host lists are validated, a matrix without entries or without rows answers -1
    with pytest.raises(IndexError):
        dev.csr_find(adj, q)
    assert np.array_equal(dev.csr_find(adj, q[(want >= 0)][:100]).cpu().numpy(), want[want >= 0][:100])
    assert dev.csr_find(adj, np.zeros((0, 2), np.int64)).shape == (0,)
    hollow = DeviceAdjacency.from_scipy(sp.csr_matrix((5, 5), dtype=np.float32), device=cuda)
    assert bool((dev.csr_find(hollow, torch.tensor([[0, 0], [4, 4], [-1, -1], [5, 0]], device=cuda)) == -1).all())
    no_rows = DeviceAdjacency(torch.zeros(1, dtype=torch.int64, device=cuda), torch.empty(0, dtype=torch.int32, device=cuda),
                              torch.empty(0, dtype=torch.float32, device=cuda), (0, 0))
    assert bool((dev.csr_find(no_rows, torch.tensor([[0, 0], [-1, -1]], device=cuda)) == -1).all())


def test_csr_find_splits_long_lists(cuda, monkeypatch):
    a = find_matrix()
    q = find_queries(a)[:1000]
    adj = DeviceAdjacency.from_scipy(a, device=cuda)
    dq = torch.from_numpy(q).to(cuda)
    whole = dev.csr_find(adj, dq)
    monkeypatch.setattr(dev, "EDGE_DOT_MAX_EDGES", 300)                          # 300 + 300 + 300 + 100
    assert torch.equal(dev.csr_find(adj, dq), whole)
    e, k = dev.edge_candidates(DeviceAdjacency.from_scipy(sp.identity(50, dtype=np.float32, format="csr"), device=cuda), 3, 11, 1000)
    monkeypatch.undo()
    e1, k1 = dev.edge_candidates(DeviceAdjacency.from_scipy(sp.identity(50, dtype=np.float32, format="csr"), device=cuda), 3, 11, 1000)
    assert torch.equal(e, e1) and torch.equal(k, k1)


# ---- 2. edge_candidates -------------------------------------------------------------------------------------------------------------------
def candidate_graphs(goldens):
    yield sp.csr_matrix((np.ones(1, np.float32), ([0], [1])), shape=(2, 2))      # (0, 1) stored, (1, 0) not
    yield sp.csr_matrix((np.ones(3, np.float32), ([0, 1, 2], [2, 1, 0])), shape=(3, 3))
    yield goldens.graph("sym64")
    yield goldens.graph("pl2000")
    n = 1000003                                                                  # no power of two; the row pointers are 8 MB
    for seed in (1, 2):                                                          # a handful of edges: candidates of the stream itself
        p = common.candidate_pairs(n, seed, 0, 5000)[[3, 10, 77, 1233, 1234, 4999]]
        yield sp.csr_matrix((np.ones(len(p), np.float32), (p[:, 0], p[:, 1])), shape=(n, n))


def test_edge_candidates_against_the_numpy_mirror(cuda, goldens):
    for k, a in enumerate(candidate_graphs(goldens)):
        n = a.shape[0]
        stored = common.stored_set(a)
        adj = DeviceAdjacency.from_scipy(a, device=cuda)
        for seed in (1, 2):
            pairs = common.candidate_pairs(n, seed, 0, 5000)
            keys = common.candidate_keys(stored, n, pairs)
            e, key = dev.edge_candidates(adj, seed, 0, 5000)
            assert e.dtype == key.dtype == torch.int64 and e.shape == (5000, 2) and key.shape == (5000,)
            assert np.array_equal(e.cpu().numpy(), pairs) and np.array_equal(key.cpu().numpy(), keys), (n, seed)
            if n <= 2000 or seed == 1 + (k % 2):
                assert (keys < 0).any(), n                                       # the refusals are really exercised
            # any division of the range gives the same bytes
            e1, k1 = dev.edge_candidates(adj, seed, 0, 1234)
            e2, k2 = dev.edge_candidates(adj, seed, 1234, 5000 - 1234)
            assert torch.equal(torch.cat((e1, e2)), e) and torch.equal(torch.cat((k1, k2)), key), (n, seed)
        # far into the stream
        first = 2 ** 40
        pairs = common.candidate_pairs(n, 2, first, 1000)
        e, key = dev.edge_candidates(adj, 2, first, 1000)
        assert np.array_equal(e.cpu().numpy(), pairs) and np.array_equal(key.cpu().numpy(), common.candidate_keys(stored, n, pairs)), n
        # the raw entry: guards around both outputs, both alignments of the pair list, a count that fills no block
        for count, odd in ((1, False), (1001, False), (1001, True)):
            pairs = common.candidate_pairs(n, 1, 7, count)
            ebuf, elead = guarded(2 * count, cuda, odd)
            kbuf, klead = guarded(count, cuda)
            dev._call(cuda, "sgl_edge_candidates", _lib.ptr(adj.rowptr), _lib.ptr(adj.col), n, 1, 7, count,
                      c_void_p(ebuf.data_ptr() + 8 * elead), c_void_p(kbuf.data_ptr() + 8 * klead))
            torch.cuda.synchronize()
            assert np.array_equal(ebuf[elead:elead + 2 * count].cpu().numpy().reshape(-1, 2), pairs), (n, count, odd)
            assert np.array_equal(kbuf[klead:klead + count].cpu().numpy(), common.candidate_keys(stored, n, pairs)), (n, count, odd)
            assert guards_intact(ebuf, elead, 2 * count) and guards_intact(kbuf, klead, count), (n, count, odd)
    assert dev.edge_candidates(adj, 1, 5, 0)[0].shape == (0, 2)
    with pytest.raises(ValueError):
        dev.edge_candidates(adj, 1, -1, 5)


# ---- 3. - 8. mask_test_edges --------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle(name, adj, seed, negatives=common.SETS):
    key = (name, seed, tuple(negatives))
    if key not in _ORACLE:
        _ORACLE[key] = common.oracle_split(adj, seed, negatives)[0]
    return _ORACLE[key]


def graph(goldens, name):
    if name == "weighted40":
        return common.weighted40()
    if name == "half_dense8":
        return common.half_dense8()
    return goldens.graph(name)


def assert_equal_splits(got, want, what):
    assert isinstance(got, EdgeSplit)
    a, b = got.adj_train.to_scipy(), want[0]
    assert a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), what
    assert a.data.dtype == np.float32 and np.array_equal(a.data, b.data), what
    for field, x, y in zip(EdgeSplit._fields[1:], got[1:], want[1:]):
        assert x.is_cuda and x.dtype == torch.int64 and x.dim() == 2 and x.shape[1] == 2, (what, field)
        assert np.array_equal(x.cpu().numpy(), y), (what, field)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("name", ["sym64", "pl2000", "dir40", "weighted40"])
def test_mask_test_edges_equals_the_sequential_oracle(cuda, goldens, name, seed):
    adj = graph(goldens, name)
    want = oracle(name, adj, seed)
    got = mask_test_edges(adj, seed=seed, device=cuda)
    assert_equal_splits(got, want, (name, seed))
    common.check_split(adj, got, strict_val=True)
    assert_equal_splits(mask_test_edges(adj, seed=seed, device=cuda, round_size=37), want, (name, seed, "rounds of 37"))
    # a DeviceAdjacency goes in as it is; the result unpacks like the reference's 7-tuple
    adj_train, train_edges, train_false, val_edges, val_false, test_edges, test_false = \
        mask_test_edges(DeviceAdjacency.from_scipy(adj, device=cuda), seed=seed)
    assert torch.equal(train_false, got.train_edges_false) and torch.equal(test_edges, got.test_edges)
    assert torch.equal(adj_train.col, got.adj_train.col)


def test_subsets_of_the_negative_sets(cuda, goldens):
    for name in ("sym64", "pl2000"):
        adj = graph(goldens, name)
        for sets in (("test",), ("val", "test"), ()):
            want = oracle(name, adj, 1, sets)
            got = mask_test_edges(adj, seed=1, device=cuda, negatives=sets)
            assert_equal_splits(got, want, (name, sets))
            common.check_split(adj, got, negatives=sets)
            assert got.train_edges_false.shape == (0, 2) and (("val" in sets) or got.val_edges_false.shape == (0, 2))
    with pytest.raises(ValueError):
        mask_test_edges(adj, device=cuda, negatives=("test", "all"))


def test_half_dense_graph_takes_every_admissible_pair_and_the_two_errors(cuda):
    adj = common.half_dense8()
    stored = common.stored_set(adj)
    admissible = sorted((i, j) for i in range(8) for j in range(i + 1, 8) if (i, j) not in stored)
    assert len(admissible) == 14
    for seed in (1, 2, 3, 4, 5):
        got = mask_test_edges(adj, seed=seed, device=cuda)
        assert_equal_splits(got, oracle("half_dense8", adj, seed), seed)
        false = torch.cat((got.train_edges_false, got.test_edges_false, got.val_edges_false)).cpu().numpy()
        assert sorted((min(i, j), max(i, j)) for i, j in false.tolist()) == admissible
        assert_equal_splits(mask_test_edges(adj, seed=seed, device=cuda, round_size=5), oracle("half_dense8", adj, seed), (seed, 5))
    with pytest.raises(ValueError):
        mask_test_edges(common.half_dense8(extra=True), seed=1, device=cuda)      # 15 needed, 13 pairs left
    with pytest.raises(RuntimeError):
        mask_test_edges(adj, seed=1, device=cuda, max_draws=5)
    with pytest.raises(RuntimeError):
        mask_test_edges(adj, seed=1, device=cuda, max_draws=60)                   # seed 1 needs 78 candidates
    assert_equal_splits(mask_test_edges(adj, seed=1, device=cuda, max_draws=78, round_size=7), oracle("half_dense8", adj, 1), "78")
    with pytest.raises(ValueError):
        mask_test_edges(sp.csr_matrix((3, 4), dtype=np.float32), device=cuda)


def test_has_edges_on_pl2000(cuda, goldens):
    adj = goldens.graph("pl2000")
    coo = common.canonical(adj).tocoo()
    stored = np.stack((coo.row, coo.col), 1).astype(np.int64)
    dadj = DeviceAdjacency.from_scipy(adj, device=cuda)
    split = mask_test_edges(dadj, seed=1)
    false = torch.cat((split.train_edges_false, split.test_edges_false, split.val_edges_false))
    for a in (adj, dadj):
        yes, no = has_edges(a, stored, device=cuda), has_edges(a, false, device=cuda)
        assert yes.dtype == torch.bool and yes.is_cuda and yes.shape == (len(stored),) and bool(yes.all())
        assert no.shape == (len(false),) and not bool(no.any())
        assert bool(has_edges(a, split.test_edges, device=cuda).all())
        assert not bool(has_edges(split.adj_train, split.test_edges).any())       # the test edges have left the training graph
        assert bool(has_edges(split.adj_train, split.train_edges.flip(1)).all())
    mixed = torch.cat((torch.from_numpy(stored[:500]).to(cuda), false[:500]))
    assert torch.equal(has_edges(adj, mixed, device=cuda), has_edges(dadj, mixed))


def test_split_feeds_the_link_prediction_task(cuda, goldens):
    adj = goldens.graph("pl2000")
    x = hash_positive(adj.shape[0], 12, seed=41)
    split = mask_test_edges(adj, seed=1, device=cuda)
    on_device = nafs_link_prediction(split.adj_train, x, 2, split.test_edges, split.test_edges_false, r_list=(0.5, 0.3, 0), device=cuda)
    on_host = nafs_link_prediction(split.adj_train.to_scipy(), x, 2, split.test_edges.cpu(), split.test_edges_false.cpu().numpy(),
                                   r_list=(0.5, 0.3, 0), device=cuda)
    assert on_device.metrics == on_host.metrics and sorted(on_device.metrics) == [0, 1]
    assert on_device[1:5] == on_host[1:5]
    assert all(0.0 < v <= 1.0 for pair in on_device.metrics.values() for v in pair)


def test_two_runs_are_bit_equal_and_seeds_differ(cuda, goldens):
    adj = goldens.graph("pl2000")
    a, b, c = (mask_test_edges(adj, seed=s, device=cuda) for s in (1, 1, 2))
    for x, y, z in zip(a[1:], b[1:], c[1:]):
        assert torch.equal(x, y)
        assert x.shape == z.shape and not torch.equal(x, z)
    assert torch.equal(a.adj_train.rowptr, b.adj_train.rowptr) and torch.equal(a.adj_train.col, b.adj_train.col)
    assert not torch.equal(a.adj_train.col, c.adj_train.col)

"""Shared by the edge-split tests (csrc/sgl_edge_split.hip, tricks/link_prediction.py: has_edges, mask_test_edges): the graphs, a
numpy mirror of the candidate stream, a SEQUENTIAL oracle -- the reference's literal loop with Python sets (sgl/tasks/utils.py:181-236)
over that stream, and the argsort split -- and check_split, which asserts the invariants the reference's own output has."""
import numpy as np
import scipy.sparse as sp

from sgl_amd.synthetic import _hash4, _mulhi64

SHUFFLE_STREAM, CANDIDATE_STREAM = 101, 102
SETS = ("train", "test", "val")                      # the reference's order of filling


def weighted40():
    """directed, weighted, n = 40, with a stored diagonal and explicitly stored zeros (on and off the diagonal)"""
    rng = np.random.default_rng(40)
    n, m = 40, 260
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    v = rng.uniform(-2.0, 2.0, m).astype(np.float32)
    v[::7] = 0.0                                     # explicit zeros
    d = np.arange(0, n, 3)
    a = sp.csr_matrix((np.concatenate((v, np.where(d % 2 == 0, 1.5, 0.0).astype(np.float32))),
                       (np.concatenate((r, d)), np.concatenate((c, d)))), shape=(n, n))
    a.sum_duplicates()
    assert (a.data == 0).any() and a.diagonal().any()
    return a


def half_dense8(extra=False):
    """n = 8 holding exactly 14 of the 28 pairs, symmetrised: E = 14, so 13 + 1 + 0 = 14 negatives are ALL the admissible pairs.
    extra=True: one more edge, one admissible pair fewer than needed."""
    pairs = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    take = [p for k, p in enumerate(pairs) if k % 2 == 0] + ([pairs[1]] if extra else [])
    r, c = np.array(take).T
    a = sp.csr_matrix((np.ones(len(take), np.float32), (r, c)), shape=(8, 8))
    return (a + a.T).tocsr()


def canonical(adj):
    a = sp.csr_matrix(adj).copy()
    a.sum_duplicates()
    a.sort_indices()
    return a


def positive_entries(adj):
    """(rows, cols) int64 of the stored off-diagonal non-zero entries in CSR order"""
    a = canonical(adj)
    rows = np.repeat(np.arange(a.shape[0], dtype=np.int64), np.diff(a.indptr))
    cols = a.indices.astype(np.int64)
    keep = (rows != cols) & (a.data != 0)
    return rows[keep], cols[keep]


def candidate_pairs(n, seed, first, count):
    """candidates first .. first + count - 1 of the stream: int64 [count, 2]"""
    t = np.arange(count, dtype=np.uint64) + np.uint64(first)
    i = _mulhi64(_hash4(seed, CANDIDATE_STREAM, t, 0), np.uint64(n))
    j = _mulhi64(_hash4(seed, CANDIDATE_STREAM, t, 1), np.uint64(n))
    return np.stack((i, j), 1).astype(np.int64)


def candidate_keys(stored, n, pairs):
    """min * n + max where i != j and (i, j) is not in the set `stored`, else -1"""
    out = np.full(len(pairs), -1, np.int64)
    for q, (i, j) in enumerate(pairs.tolist()):
        if i != j and (i, j) not in stored:
            out[q] = min(i, j) * n + max(i, j)
    return out


def stored_set(adj):
    a = canonical(adj).tocoo()
    return set(zip(a.row.tolist(), a.col.tolist()))


def oracle_split(adj, seed, negatives=SETS):
    """(the seven outputs as numpy / scipy, candidates drawn).  The split is the stable argsort of the shuffle hashes; the negatives
    are the reference's loop, one candidate at a time, over the stream."""
    n = adj.shape[0]
    rows, cols = positive_entries(adj)
    up = rows < cols
    edges = np.stack((rows[up], cols[up]), 1)
    e = len(edges)
    num_test, num_val = e // 10, e // 20
    order = np.argsort(_hash4(seed, SHUFFLE_STREAM, np.arange(e, dtype=np.uint64), 0), kind="stable")
    val_edges, test_edges = edges[order[:num_val]], edges[order[num_val:num_val + num_test]]
    train_edges = np.delete(edges, order[:num_val + num_test], axis=0)
    t = sp.csr_matrix((np.ones(len(train_edges), np.float32), (train_edges[:, 0], train_edges[:, 1])), shape=(n, n))
    adj_train = (t + t.T).tocsr()

    edges_all_set = set(zip(rows.tolist(), cols.tolist()))
    sizes = {"train": len(train_edges), "test": num_test, "val": num_val}
    accepted, false, drawn, block = set(), {}, 0, []
    for name in SETS:
        got = []
        while name in negatives and len(got) < sizes[name]:
            if not block:
                block = candidate_pairs(n, seed, drawn, 4096).tolist()[::-1]
            i, j = block.pop()
            drawn += 1
            if i == j or (i, j) in edges_all_set or (i, j) in accepted or (j, i) in accepted:
                continue
            accepted.add((i, j))
            got.append((i, j))
        false[name] = np.array(got, np.int64).reshape(-1, 2)
    return (adj_train, train_edges, false["train"], val_edges, false["val"], test_edges, false["test"]), drawn


def to_host(x):
    if hasattr(x, "to_scipy"):
        return x.to_scipy()
    if hasattr(x, "cpu"):
        return x.cpu().numpy()
    return x


def check_split(adj, split, strict_val=True, negatives=SETS):
    """the invariants of mask_test_edges' output (the reference's own passes with strict_val=False: its val negatives may repeat)"""
    adj_train, train, train_f, val, val_f, test, test_f = (to_host(x) for x in split)
    n = adj.shape[0]
    rows, cols = positive_entries(adj)
    up = rows < cols
    e = int(up.sum())
    num_test, num_val = e // 10, e // 20
    sizes = {"train": e - num_test - num_val, "test": num_test, "val": num_val}
    lists = {"train": (train, train_f), "test": (test, test_f), "val": (val, val_f)}
    for name, (p, f) in lists.items():
        p, f = np.asarray(p).reshape(-1, 2), np.asarray(f).reshape(-1, 2)
        lists[name] = (p, f)
        assert len(p) == sizes[name], (name, len(p), sizes[name])
        assert len(f) == (sizes[name] if name in negatives else 0), (name, len(f))
    # a partition of the row < col positives
    parts = np.concatenate([lists[s][0] for s in SETS])
    assert sorted(map(tuple, parts.tolist())) == sorted(zip(rows[up].tolist(), cols[up].tolist()))
    # adj_train = T + T^T with ones
    tr = lists["train"][0]
    t = sp.csr_matrix((np.ones(len(tr)), (tr[:, 0], tr[:, 1])), shape=(n, n))
    want, got = canonical(t + t.T), canonical(sp.csr_matrix(adj_train))
    assert got.shape == (n, n) and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data, np.ones(got.nnz, got.data.dtype))
    # negatives: no self pair, not stored as drawn, no key twice inside a set or between sets
    stored = set(zip(rows.tolist(), cols.tolist()))
    seen = set()
    for name in SETS:
        f = lists[name][1]
        assert f.size == 0 or (f.min() >= 0 and f.max() < n)
        mine = []
        for i, j in f.tolist():
            assert i != j and (i, j) not in stored, (name, i, j)
            mine.append((min(i, j), max(i, j)))
        if strict_val or name != "val":
            assert len(set(mine)) == len(mine), f"{name}: a pair twice"
        assert not (set(mine) & seen), f"{name}: shares a pair with an earlier set"
        seen |= set(mine)

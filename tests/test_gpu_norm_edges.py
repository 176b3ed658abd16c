"""Normalisation of zero, cancelling and negative weights on a real MI355X: run with `-m gpu`.

The fixture tests/golden/g15_norm_edges.npz (make_g15_norm_edges.py) holds what the reference's scipy pipeline makes of two 48-node
graphs with stored zeros, a_ii = -1, zero degrees and one negative degree: scipy stores no exact zero, so the pattern of A_hat
depends on (r, alpha) and is recorded per variant.  Every Python route to A_hat must return that pattern, those values and NaN at
those places; the fixture never leaves the first workgroup of any kernel, so one graph of 1100 nodes with the same kinds of nodes on
the row-tile edges of the build (256 rows) and scale (512 rows) kernels is compared with the CPU oracle, itself pinned to the
fixture by tests/test_oracle_golden.py.

Tolerances are the ones the suite already uses for normalisation (test_device_normalisation_matches_reference_goldens): pattern bit
for bit, fp64 within 1e-14 relative, fp32 bit-equal to the reference's rounding with the host's pow(), within 1.2e-7 relative
(1 ulp) with the device's; NaN positions identical."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import oracle
from sgl_amd import _lib
from sgl_amd import device as dev

pytestmark = pytest.mark.gpu

G1_VARIANTS = [("lap", r, None) for r in (0.0, 0.3, 0.5, 1.0)] + \
              [("ppr", 0.5, a) for a in (0.1, 0.15, 0.2, 0.3)] + [("ppr", 0.3, 0.15)]
G15_VARIANTS = G1_VARIANTS + [("ppr", 0.5, 1.0)]  # alpha = 1: (1 - alpha) A_hat is all zeros (and NaNs); recorded in the fixture too
SWEEP = [("ppr", 0.5, 0.1), ("ppr", 0.5, 0.15), ("lap", 0.5, None), ("ppr", 0.5, 0.3), ("lap", 0.3, None), ("ppr", 0.3, 0.15),
         ("ppr", 0.5, 0.2)]                      # the order of test_prepared_block_serves_an_r_alpha_sweep
G15_BOUNDS = ([0, 48], [0, 17, 17, 40, 48])      # one block; an EMPTY block and cuts next to / on special nodes
BIG_BOUNDS = [0, 256, 256, 700, 1100]
BIG_VARIANTS = [("lap", 0.0, None), ("lap", 0.5, None), ("ppr", 0.3, 0.15)]


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def key_of(gname, kind, r, a):
    return f"{gname}|{kind}|{r}" + ("" if a is None else f"|{a}")


def transpose(csr):
    """(indptr, indices, data) of the transposed matrix, every stored zero kept (numpy only)"""
    ptr, col, val = csr
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    order = np.lexsort((rows, col))
    t_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=t_ptr[1:])
    return t_ptr, rows[order].astype(np.int32), val[order]


def mirror_zeros(csr):
    """the same matrix with every stored off-diagonal zero stored on the other side too: symmetric in stored pattern as well.  The
    reference's result is unchanged -- scipy drops every stored zero at A + I"""
    ptr, col, val = csr
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    have = set(zip(rows.tolist(), col.tolist()))
    add = [(c, r_) for r_, c, v in zip(rows.tolist(), col.tolist(), val.tolist()) if v == 0 and (c, r_) not in have]
    assert add
    rows = np.concatenate([rows, [a[0] for a in add]])
    cols = np.concatenate([col, [a[1] for a in add]])
    vals = np.concatenate([val, np.zeros(len(add), val.dtype)])
    order = np.lexsort((cols, rows))
    out = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=out[1:])
    return out, cols[order].astype(np.int32), vals[order]


def upload(csr, cuda):
    ptr, col, val = csr
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(cuda)  # noqa: E731
    return to(ptr, np.int64), to(col, np.int32), to(val, np.float32)


def rows_of(csr, lo, hi):
    ptr, col, val = csr
    return ptr[lo:hi + 1].astype(np.int64) - int(ptr[lo]), col[ptr[lo]:ptr[hi]], val[ptr[lo]:ptr[hi]]


def host(result):
    return tuple(t.cpu().numpy() for t in result)


def check(got, ref, what, bits32=True):
    """got = (ptr, col, v32, v64) as numpy, ref = (ptr, col, fp64 values): the suite's normalisation tolerances"""
    ptr, col, v32, v64 = got
    r_ptr, r_col, r_val = ref
    assert np.array_equal(ptr, r_ptr), (what, "row pointers", int(ptr[-1]), int(r_ptr[-1]))
    assert np.array_equal(col, r_col), (what, "columns")
    nan = np.isnan(r_val)
    assert np.array_equal(np.isnan(v64), nan) and np.array_equal(np.isnan(v32), nan), (what, "NaN positions")
    assert not (v64 == 0).any(), (what, "a stored zero")
    f = ~nan
    rel = np.abs(v64[f] - r_val[f]) / np.maximum(np.abs(r_val[f]), 1e-300)
    assert rel.size == 0 or rel.max() <= 1e-14, (what, float(rel.max()))
    r32 = r_val.astype(np.float32)
    if bits32:
        assert np.array_equal(v32[f], r32[f]), (what, int((v32[f] != r32[f]).sum()))
    else:
        assert np.allclose(v32[f], r32[f], rtol=1.2e-7, atol=0), what


def concat_blocks(parts):
    """row blocks (local row pointers) laid end to end"""
    offs = np.concatenate([[0], np.cumsum([p[0][-1] for p in parts])])
    ptr = np.concatenate([p[0][:-1] + o for p, o in zip(parts, offs[:-1])] + [offs[-1:]])
    return (ptr,) + tuple(np.concatenate([p[k] for p in parts]) for k in (1, 2, 3))


def global_degrees(dcsr, n, cuda):
    deg = torch.empty(n, dtype=torch.float64, device=cuda)
    _lib.check(_lib.lib().sgl_norm_degrees(n, 0, _lib.ptr(dcsr[0]), _lib.ptr(dcsr[1]), _lib.ptr(dcsr[2]), _lib.ptr(deg),
                                           _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    return deg


def blocks(t_csr, bounds, n, r, a, symmetric, deg, cuda):
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        rp, cc, vv = upload(rows_of(t_csr, lo, hi), cuda)
        parts.append(host(dev.normalize_block(rp, cc, vv, lo, n, r, a, symmetric=symmetric, return_fp64=True,
                                              deg=deg if len(bounds) > 2 else None)))
    return concat_blocks(parts)


@pytest.fixture(scope="module")
def g15(goldens):
    z = goldens.npz("g15_norm_edges")
    graphs = {name: (z[name + "|indptr"], z[name + "|indices"], z[name + "|data"]) for name in ("edge48", "edge48s")}
    graphs["edge48m"] = mirror_zeros(graphs["edge48s"])
    for csr in graphs.values():
        assert (csr[2] == 0).sum() >= 4                              # the stored zeros reach the device

    def ref(gname, kind, r, a):
        k = key_of("edge48s" if gname == "edge48m" else gname, kind, r, a)
        return z[k + "|indptr"], z[k + "|indices"], z[k + "|data"]
    return z, graphs, ref


@pytest.mark.parametrize("gname", ["edge48", "edge48s", "edge48m"])
def test_whole_matrix_routes_match_g15(g15, cuda, gname):
    """adj_to_symmetric_norm[_device], normalize_adj with the host's pow (PreparedAdjacency: the symmetric route for edge48m, the
    transposed PreparedBlock for edge48 and for edge48s -- its one-sided stored zeros make its PATTERN asymmetric), with the
    device's pow (sgl_norm_prepare / sgl_norm_execute) and with "auto" """
    from sgl_amd.operators.utils import adj_to_symmetric_norm, adj_to_symmetric_norm_device
    _, graphs, ref = g15
    csr = graphs[gname]
    n = len(csr[0]) - 1
    mat = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n))
    assert mat.nnz == len(csr[2])
    d = upload(csr, cuda)
    prep = dev.PreparedAdjacency(*d, n)
    assert prep.symmetric == (gname == "edge48m") and prep.may_hold_zero
    for kind, r, a in G15_VARIANTS:
        want = ref(gname, kind, r, a)
        what = key_of(gname, kind, r, a)
        check(host(adj_to_symmetric_norm_device(mat, r, a, device=cuda, return_fp64=True)), want, (what, "scipy in"))
        check(host(dev.normalize_adj(*d, n, r, a, return_fp64=True, host_pow=True)), want, (what, "host pow"))
        check(host(prep.normalize(r, a, return_fp64=True)), want, (what, "prepared"))
        p3 = prep.normalize(r, a)                                     # without the fp64 values: the same pattern and fp32 bits
        assert len(p3) == 3 and np.array_equal(p3[0].cpu().numpy(), want[0]) and np.array_equal(p3[1].cpu().numpy(), want[1])
        assert np.array_equal(p3[2].cpu().numpy(), want[2].astype(np.float32), equal_nan=True), what
        check(host(dev.normalize_adj(*d, n, r, a, return_fp64=True, host_pow=False)), want, (what, "device pow"), bits32=False)
        dev.clear_power_cache()
        before = dev.pow_stats["device"]
        auto = host(dev.normalize_adj(*d, n, r, a, return_fp64=True, host_pow="auto"))
        check(auto, want, (what, "auto"), bits32=dev.pow_stats["device"] == before)
        if a is None:
            s = adj_to_symmetric_norm(mat, r)                         # the reference's own signature: a scipy matrix, fp64
            assert np.array_equal(s.indptr, want[0]) and np.array_equal(s.indices, want[1]), what
            assert s.data.dtype == np.float64 and np.array_equal(np.isnan(s.data), np.isnan(want[2])), what
            assert np.allclose(s.data, want[2], rtol=1e-14, atol=0, equal_nan=True), what


@pytest.mark.parametrize("gname,symmetric", [("edge48", False), ("edge48s", False), ("edge48s", True), ("edge48m", True)])
def test_row_blocks_match_g15(g15, cuda, gname, symmetric):
    """normalize_block on the rows of T = A^T (symmetric=True: of A itself -- a value-symmetric A whose stored zeros are one-sided
    included): laid end to end the blocks are the whole-matrix result bit for bit, and the fixture"""
    _, graphs, ref = g15
    csr = graphs[gname]
    n = len(csr[0]) - 1
    d = upload(csr, cuda)
    deg = global_degrees(d, n, cuda)
    t = csr if symmetric else transpose(csr)
    for kind, r, a in G15_VARIANTS:
        full = host(dev.normalize_adj(*d, n, r, a, return_fp64=True))
        for bounds in G15_BOUNDS:
            got = blocks(t, bounds, n, r, a, symmetric, deg, cuda)
            what = (key_of(gname, kind, r, a), symmetric, len(bounds))
            check(got, ref(gname, kind, r, a), what)
            for g_, f_ in zip(got, full):
                assert np.array_equal(g_, f_, equal_nan=True), what


@pytest.mark.parametrize("gname", ["edge48", "edge48m"])
def test_r_alpha_sweep_serves_the_cached_laplacian_g15(g15, cuda, gname):
    """a PPR sweep keeps the UNCOMPACTED fp64 Laplacian of its r and mixes it per alpha (sgl_norm_block_mix_at at the diagonal
    positions of the uncompacted block); what is returned is compacted per request: the cached and the one-pass route give the
    same bits, both the fixture's -- for a proper row block and for a whole PreparedAdjacency"""
    _, graphs, ref = g15
    csr = graphs[gname]
    n = len(csr[0]) - 1
    symmetric = gname == "edge48m"
    d = upload(csr, cuda)
    deg = global_degrees(d, n, cuda)
    lo, hi = 17, 40
    blk = upload(rows_of(csr if symmetric else transpose(csr), lo, hi), cuda)
    prep_b = dev.PreparedBlock(*blk, lo, n, symmetric=symmetric, deg=deg)
    prep_a = dev.PreparedAdjacency(*d, n)
    assert prep_b.may_hold_zero and prep_a.may_hold_zero
    for kind, r, a in SWEEP:
        w_ptr, w_col, w_val = ref(gname, kind, r, a)
        a0, a1 = int(w_ptr[lo]), int(w_ptr[hi])
        want_b = (w_ptr[lo:hi + 1] - a0, w_col[a0:a1], w_val[a0:a1])
        what = key_of(gname, kind, r, a)
        got = prep_b.normalize(r, a, return_fp64=True)
        check(host(got), want_b, (what, "block sweep"))
        one = dev.normalize_block(*blk, lo, n, r, a, symmetric=symmetric, deg=deg, return_fp64=True)
        assert all(torch.equal(x_, y_) or np.array_equal(x_.cpu().numpy(), y_.cpu().numpy(), equal_nan=True)
                   for x_, y_ in zip(got, one)), what
        got = prep_a.normalize(r, a, return_fp64=True)
        check(host(got), (w_ptr, w_col, w_val), (what, "whole sweep"))
        one = dev.normalize_adj(*d, n, r, a, return_fp64=True)
        assert all(np.array_equal(x_.cpu().numpy(), y_.cpu().numpy(), equal_nan=True) for x_, y_ in zip(got, one)), what
    assert prep_b._hat64[0][0] == 0.5 and prep_b._hat64[1].numel() == prep_b.nnz_out     # the cache entry stays uncompacted


@pytest.mark.parametrize("gname", ["edge48", "edge48s"])
def test_graph_ops_match_recorded_hops_g15(g15, cuda, gname):
    """LaplacianGraphOp / PprGraphOp in strict order on the finite x and on the one with inf in rows 31 and 41, which other rows
    reach only through a zero degree factor or a zero-weight edge: every hop bit-equal to the reference's (NaN at the same places),
    the set of non-finite rows the fixture's"""
    from sgl_amd.operators import base_op
    from sgl_amd.operators.graph_op import LaplacianGraphOp, PprGraphOp
    z, graphs, _ = g15
    csr = graphs[gname]
    n = len(csr[0]) - 1
    mat = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n))
    base_op.clear_graph_cache()
    try:
        for kind, r, a in (("lap", 0.5, None), ("ppr", 0.5, 0.15)):
            for xname in ("fin", "inf"):
                x = z["x_" + xname]
                op = LaplacianGraphOp(2, r=r, strict_order=True) if kind == "lap" else PprGraphOp(2, r=r, alpha=a, strict_order=True)
                hops = op.propagate(mat, x.copy())
                assert len(hops) == 3 and np.array_equal(hops[0].cpu().numpy(), x)
                for h in (1, 2):
                    want = z[f"{key_of(gname, kind, r, a)}|{xname}|h{h}"]
                    got = hops[h].cpu().numpy()
                    what = (gname, kind, xname, h)
                    bad_got, bad_want = ~np.isfinite(got).all(1), ~np.isfinite(want).all(1)
                    assert np.array_equal(bad_got, bad_want), (what, np.nonzero(bad_got ^ bad_want)[0])
                    assert np.array_equal(got, want, equal_nan=True), what
    finally:
        base_op.clear_graph_cache()


def test_alpha_one_leaves_the_identity_of_an_ordinary_graph(goldens, cuda):
    """(1 - alpha) = 0 exactly: every (finite) entry of A_hat becomes 0, which scipy's sum with alpha I does not store, and the
    diagonal 0 + 1 -- the one request that drops entries of a graph of positive weights"""
    g = goldens.graph("pl256")
    n = g.shape[0]
    d = upload((g.indptr, g.indices, g.data), cuda)
    prep = dev.PreparedAdjacency(*d, n)
    assert not prep.may_hold_zero
    want = tuple(np.asarray(v) for v in oracle.sym_norm_csr(g.indptr, g.indices, g.data, n, 0.5, 1.0))
    assert np.array_equal(want[0], np.arange(n + 1)) and np.array_equal(want[1], np.arange(n)) and (want[2] == 1.0).all()
    for host_pow in (True, False):
        check(host(dev.normalize_adj(*d, n, 0.5, 1.0, return_fp64=True, host_pow=host_pow)), want, host_pow)
    check(host(prep.normalize(0.5, 1.0, return_fp64=True)), want, "prepared")
    check(host(dev.normalize_block(*d, 0, n, 0.5, 1.0, return_fp64=True)), want, "block")


# ---- one larger shape against the oracle ---------------------------------------------------------------------------------------
BIG_N = 1100


def big_graph(symmetric):
    """directed weighted graph of 1100 nodes, average degree about 6 (symmetric=True: its symmetrisation, stored zeros mirrored
    too), with the fixture's kinds of nodes on the row-tile edges of the build (256) and scale (512) kernels:
      0     a_ii = -1 plus ordinary edges              255   only a_ii = -1 (its row of A + I is empty)
      256   degree 0 through an off-diagonal -1        511   stored zeros: off the diagonal, on it, and a cancelled pair
      512   degree -2, neighbours of positive degree   1023, 1024   two adjacent zero-degree nodes
      1099  a_ii = -1 and one stored zero: degree 0
    and a hub row (600) and a hub column (700) of more than 64 entries, each with a cancelled diagonal and stored zeros (the
    cooperative row sum of block_build_kernel)"""
    rng = np.random.default_rng(1100)
    special = {255, 256, 512, 1023, 1024, 1099, 600, 700}
    pool = np.array([i for i in range(BIG_N) if i not in special])
    rows, cols, vals = [], [], []

    def add(i, j, w, where="both"):
        if symmetric or where in ("out", "both"):
            rows.append(i); cols.append(j); vals.append(w)
        if (symmetric or where in ("in", "both")) and i != j:
            rows.append(j); cols.append(i); vals.append(w)

    planted = [(0, 1, 1.0, "both"), (0, 3, 0.5, "out"),
               (256, 260, -1.0, "out"), (256, 261, 2.0, "out"), (256, 262, -2.0, "out"), (256, 263, 0.5, "in"), (256, 264, -0.5, "in"),
               (260, 261, 2.5, "both"), (261, 262, 2.5, "both"), (260, 262, 2.5, "both"), (263, 264, 2.0, "both"),
               (511, 520, 0.0, "both"), (511, 521, 1.5, "out"), (511, 521, -1.5, "out"), (511, 522, 1.0, "both"),
               (512, 530, -1.5, "out"), (512, 531, -1.5, "out"), (512, 532, 1.0, "in"), (512, 533, -1.0, "in"),
               (530, 531, 3.0, "both"), (532, 533, 3.0, "both"),
               (1023, 1024, -1.0, "both"), (1099, 5, 0.0, "both"), (700, 2, 1.0, "out")]
    taken = {(min(i, j), max(i, j)) for i, j, _, _ in planted}
    hub_nb = rng.choice(pool[pool > 40], 150, replace=False)
    for k, j in enumerate(hub_nb[:75]):                              # hub row 600: 75 entries, three of them stored zeros
        add(600, int(j), 0.0 if k % 25 == 0 else float(np.float32(rng.uniform(0.25, 3.0))), "out")
        taken.add((min(600, int(j)), max(600, int(j))))
    for k, i in enumerate(hub_nb[75:]):                              # hub column 700
        add(700, int(i), 0.0 if k % 25 == 0 else float(np.float32(rng.uniform(0.25, 3.0))), "in")
        taken.add((min(700, int(i)), max(700, int(i))))
    for i, j, w, where in planted:
        add(i, j, w, where)
    for i, w in ((0, -1.0), (255, -1.0), (1099, -1.0), (600, -1.0), (700, -1.0), (511, 0.0), (7, 1.25)):
        add(i, i, w)
    for _ in range(6400 if not symmetric else 3200):
        i, j = (int(v) for v in rng.choice(pool, 2, replace=False))
        if (min(i, j), max(i, j)) in taken:
            continue
        taken.add((min(i, j), max(i, j)))
        add(i, j, float(np.float32(rng.uniform(0.25, 3.0))), "out")
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals, np.float32)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    new = np.ones(len(rows), dtype=bool)
    new[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    data = np.zeros(int(new.sum()), dtype=np.float32)
    np.add.at(data, np.cumsum(new) - 1, vals)                        # duplicates summed, stored zeros kept
    ptr = np.zeros(BIG_N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[new], minlength=BIG_N), out=ptr[1:])
    return ptr, cols[new].astype(np.int32), data


@pytest.fixture(scope="module")
def big():
    out = {}
    for name, symmetric in (("dir", False), ("sym", True)):
        csr = big_graph(symmetric)
        ptr, col, val = csr
        dense = sp.csr_matrix((val.astype(np.float64), col, ptr), shape=(BIG_N, BIG_N)).toarray()
        deg = (dense + np.eye(BIG_N)).sum(1)
        assert sorted(np.nonzero(deg == 0)[0]) == [255, 256, 1023, 1024, 1099] and list(np.nonzero(deg < 0)[0]) == [512]
        nb = set(np.nonzero(dense[512])[0]) | set(np.nonzero(dense[:, 512])[0])
        assert deg[512] == -2 and all(deg[j] > 0 for j in nb)       # no negative degree next to a zero degree (out of scope)
        assert (val == 0).sum() >= 8 and 5.0 < len(val) / BIG_N < 7.5
        per_row, per_col = np.diff(ptr), np.bincount(col, minlength=BIG_N)
        assert per_row[600] > 64 and per_col[700] > 64
        assert dense[600, 600] == -1 and dense[700, 700] == -1
        assert (val[ptr[600]:ptr[601]] == 0).sum() >= 3 and (dense[:, 700] == 0).sum() < BIG_N
        if symmetric:
            assert np.array_equal(dense, dense.T)
        refs = {(r, a): oracle.sym_norm_csr(ptr, col, val, BIG_N, r, a) for _, r, a in BIG_VARIANTS}
        for (r, a), ref in refs.items():
            assert np.isnan(ref[2]).any() == (r != 0.0) and ref[0][-1] < len(val) + BIG_N - 8      # it really prunes
        out[name] = (csr, refs)
    return out


@pytest.mark.parametrize("name", ["dir", "sym"])
def test_tile_edges_and_hub_rows_match_the_oracle(big, cuda, name):
    """more than one workgroup of every kernel: the special nodes sit on both sides of the 256- and 512-row tile edges, the hubs
    take the cooperative row sum; whole matrix (symmetric route / transposed route / all-device route) and row blocks with an
    empty block"""
    csr, refs = big[name]
    d = upload(csr, cuda)
    prep = dev.PreparedAdjacency(*d, BIG_N)
    assert prep.symmetric == (name == "sym") and prep.may_hold_zero
    deg = global_degrees(d, BIG_N, cuda)
    dense = sp.csr_matrix((csr[2].astype(np.float64), csr[1], csr[0]), shape=(BIG_N, BIG_N)).toarray()
    assert np.array_equal(deg.cpu().numpy(), (dense + np.eye(BIG_N)).sum(1))     # (sums of few fp32 weights: exact in fp64)
    t = csr if name == "sym" else transpose(csr)
    for kind, r, a in BIG_VARIANTS:
        want = tuple(np.asarray(v) for v in refs[(r, a)])
        what = (name, kind, r, a)
        full = host(prep.normalize(r, a, return_fp64=True))
        check(full, want, (what, "whole"))
        check(host(dev.normalize_adj(*d, BIG_N, r, a, return_fp64=True, host_pow=False)), want, (what, "device pow"), bits32=False)
        got = blocks(t, BIG_BOUNDS, BIG_N, r, a, name == "sym", deg, cuda)
        check(got, want, (what, "blocks"))
        for g_, f_ in zip(got, full):
            assert np.array_equal(g_, f_, equal_nan=True), what


def test_ordinary_graphs_never_enter_the_compaction(goldens, cuda, monkeypatch):
    """a graph of strictly positive weights has no stored zero in A + I and no zero degree: one flag per preparation says so, and
    no route ever looks for zeros to drop"""
    from sgl_amd.operators.utils import adj_to_symmetric_norm_device, canonical_csr

    def boom(*_a, **_k):
        raise AssertionError("an ordinary graph entered the zero compaction")
    monkeypatch.setattr(dev, "_drop_exact_zeros", boom)
    g = canonical_csr(goldens.graph("pl2000"))
    g1 = goldens.npz("g1_norm")
    n = g.shape[0]
    d = upload((g.indptr, g.indices, g.data), cuda)
    prep = dev.PreparedAdjacency(*d, n)
    blk = dev.PreparedBlock(*d, 0, n)
    assert prep.symmetric and not prep.may_hold_zero and not blk.may_hold_zero
    for kind, r, a in G1_VARIANTS:
        ref = g1[key_of("pl2000", kind, r, a)].astype(np.float32)
        for route in (lambda: adj_to_symmetric_norm_device(g, r, a, device=cuda), lambda: prep.normalize(r, a),
                      lambda: blk.normalize(r, a), lambda: dev.normalize_adj(*d, n, r, a, host_pow="auto")):
            p_, c_, v_ = route()
            assert int(p_[-1]) == len(ref) and np.array_equal(v_.cpu().numpy(), ref), (kind, r, a)
        assert prep.normalize(r, a)[0] is prep.rowptr and blk.normalize(r, a)[1] is blk.col      # the prepared arrays themselves
        p_, c_, v_ = dev.normalize_adj(*d, n, r, a, host_pow=False)
        assert np.allclose(v_.cpu().numpy(), ref, rtol=1.2e-7, atol=0)

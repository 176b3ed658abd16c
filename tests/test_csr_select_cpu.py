"""CPU-side checks of the CSR select (csrc/sgl_csr_select.hip, device.csr_select, sgl_amd/transforms.py): the two exported symbols and
their bindings, their refusals without a GPU -- a non-zero code and a message that names the entry, nothing launched -- the test
oracle against what the REFERENCE's transforms returned (tests/golden/g20_transforms.npz) and against scipy's a[m][:, m], the drop
threshold and the random draws, and the argument checks of the Python layer."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT

import csr_select_common as common
from sgl_amd import _lib
from sgl_amd.synthetic import _hash4

ROWPTR, FILL = "sgl_csr_select_rowptr", "sgl_csr_select_fill"
G20_GRAPHS = ("sym64", "pl256", "dir40", "symdiag48")


@pytest.mark.parametrize("name", [ROWPTR, FILL])
def test_library_exports_the_symbols(name):
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, name), f"{name} is not exported by libsgl_hip.so"
    assert name in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 108


@pytest.mark.parametrize("name,count", [(ROWPTR, 19), (FILL, 22)])
def test_header_and_binding_argument_counts_agree(name, count):
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sgl_hip.h"
    params = [p for p in m.group(1).split(",") if p.strip()]
    restype, argtypes = _lib.PROTOTYPES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == count, (len(argtypes), params)
    for word in ("d_row_map", "d_col_map", "d_entry_keep", "symmetric_mask", "drop_self", "drop_below", "seed", "symmetric", "lanes"):
        assert word in m.group(1), word


def test_the_two_entries_take_the_same_selection_arguments():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgl_hip.h")).read(), flags=re.S)
    lists = [re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text).group(1) for name in (ROWPTR, FILL)]
    cut = [" ".join(t.split())[" ".join(t.split()).index("const int32_t *d_row_map"):" ".join(t.split()).index("int lanes") + 9] for t in lists]
    assert cut[0] == cut[1], cut


def test_streams_are_listed_in_the_hash_header():
    text = open(os.path.join(ROOT, "sgl_amd", "csrc", "sgl_hash.h")).read()
    assert "103 edge drop" in text and "104 node drop" in text


def test_public_names_are_exported():
    import sgl_amd
    from sgl_amd import device as dev
    from sgl_amd import transforms as tr
    for name in ("Subgraph", "get_subgraph", "random_drop_nodes", "drop_edges", "biased_drop_edges", "random_drop_edges", "remove_self_loops",
                 "mask_features"):
        assert name in tr.__all__ and callable(getattr(tr, name))
    assert sgl_amd.transforms is tr
    assert callable(dev.csr_select) and dev.CSR_SELECT_LANES == common.LANES
    assert tr.Subgraph._fields == ("adj", "x", "y", "node_ids")
    assert (tr.EDGE_DROP_STREAM, tr.NODE_DROP_STREAM) == (common.EDGE_DROP_STREAM, common.NODE_DROP_STREAM)


class Args:
    """calls on HOST memory that is never touched: every bad call is refused before anything is launched.  A 4 x 4 matrix."""

    def __init__(self):
        self.buf = {k: (ctypes.c_int64 * 16)() for k in ("rowptr", "col", "val", "row_map", "col_map", "keep", "out_rowptr", "out_col", "out_val",
                                                          "out_pos")}
        p = {k: ctypes.cast(v, ctypes.c_void_p) for k, v in self.buf.items()}
        self.nnz_out = ctypes.c_int64(-7)
        self.base = dict(p, n_rows=4, n_cols=4, nnz=6, n_rows_out=3, n_cols_out=3, symmetric_mask=0, drop_self=0, drop_below=0, seed=1,
                         symmetric=0, lanes=0)

    @staticmethod
    def off(p, k):
        return ctypes.c_void_p(p.value + k)

    def call_rowptr(self, **change):
        k = dict(self.base, **change)
        return _lib.lib().sgl_csr_select_rowptr(k["rowptr"], k["col"], k["n_rows"], k["n_cols"], k["nnz"], k["row_map"], k["col_map"], k["n_rows_out"],
                                                k["n_cols_out"], k["keep"], k["symmetric_mask"], k["drop_self"], k["drop_below"], k["seed"],
                                                k["symmetric"], k["lanes"], k["out_rowptr"], ctypes.byref(self.nnz_out), None)

    def call_fill(self, **change):
        k = dict(self.base, **change)
        return _lib.lib().sgl_csr_select_fill(k["rowptr"], k["col"], k["val"], k["n_rows"], k["n_cols"], k["nnz"], k["row_map"], k["col_map"],
                                              k["n_rows_out"], k["n_cols_out"], k["keep"], k["symmetric_mask"], k["drop_self"], k["drop_below"],
                                              k["seed"], k["symmetric"], k["lanes"], k["out_rowptr"], k["out_col"], k["out_val"], k["out_pos"], None)


def refused(call, name, **change):
    rc = call(**change)
    msg = _lib.last_error()
    assert rc != 0, change
    assert msg and name in msg, (change, msg)


@pytest.mark.parametrize("which", [ROWPTR, FILL])
def test_bad_arguments_are_refused_without_a_gpu(which):
    a = Args()
    call = a.call_rowptr if which == ROWPTR else a.call_fill
    b = a.base
    for key in ("n_rows", "n_cols", "nnz", "n_rows_out", "n_cols_out"):
        refused(call, which, **{key: -1})
    refused(call, which, n_rows=1 << 31)
    refused(call, which, n_rows_out=1 << 31)
    refused(call, which, n_cols=1 << 31)
    refused(call, which, n_cols_out=1 << 31)
    refused(call, which, row_map=None)                       # the identity cannot shrink the matrix: n_rows_out = 3, n_rows = 4
    refused(call, which, col_map=None)
    refused(call, which, rowptr=None)
    refused(call, which, col=None)
    refused(call, which, keep=None, symmetric_mask=1)
    for lanes in (-1, 1, 2, 8, 32, 63, 65, 128):
        refused(call, which, lanes=lanes)
    refused(call, which, rowptr=a.off(b["rowptr"], 4))
    refused(call, which, col=a.off(b["col"], 2))
    refused(call, which, row_map=a.off(b["row_map"], 2))
    refused(call, which, col_map=a.off(b["col_map"], 1))
    if which == ROWPTR:
        refused(call, which, out_rowptr=None)
        refused(call, which, out_rowptr=a.off(b["out_rowptr"], 4))
        assert a.nnz_out.value == -7                          # never written by a refused call
    else:
        for key in ("val", "out_rowptr", "out_col", "out_val"):
            refused(call, which, **{key: None})
        refused(call, which, val=a.off(b["val"], 2))
        refused(call, which, out_rowptr=a.off(b["out_rowptr"], 4))
        refused(call, which, out_col=a.off(b["out_col"], 2))
        refused(call, which, out_val=a.off(b["out_val"], 2))
        refused(call, which, out_pos=a.off(b["out_pos"], 4))
        assert a.call_fill(nnz=0) == 0, _lib.last_error()     # nothing to write: no launch, no device needed
        assert a.call_fill(nnz=0, out_pos=None, keep=None) == 0, _lib.last_error()


# ---- the oracle against the reference's recorded results and against scipy -------------------------------------------------------------
@pytest.mark.parametrize("name", G20_GRAPHS)
def test_oracle_reproduces_the_reference(goldens, name):
    g = goldens.npz("g20_transforms")
    a = common.g20_graph(goldens, name)
    edge_mask, node_mask = g[f"{name}|edge_mask"], g[f"{name}|node_mask"]
    assert common.same_csr(common.oracle_matrix(a, entry_keep=edge_mask), common.recorded(goldens, f"{name}|drop"))
    assert common.same_csr(common.oracle_matrix(a, drop_self=True), common.recorded(goldens, f"{name}|noself"))
    for key, keep_ids in (("sub", False), ("sub_keep", True)):
        id_map, n_out = common.mask_to_map(node_mask, keep_ids)
        got = common.oracle_matrix(a, row_map=id_map, col_map=id_map, n_rows_out=n_out, n_cols_out=n_out)
        assert common.same_csr(got, common.recorded(goldens, f"{name}|{key}")), key
    ours = common.oracle_matrix(a, entry_keep=edge_mask, symmetric_mask=True)
    ref = common.recorded(goldens, f"{name}|drop_und")
    if name in ("sym64", "pl256"):                             # symmetric, zero diagonal: identical
        assert a.diagonal().any() == False and (a != a.T).nnz == 0      # noqa: E712
        assert common.same_csr(ours, ref)
    elif name == "symdiag48":                                  # the reference stores a kept self-loop twice: exactly double
        assert (a != a.T).nnz == 0 and np.count_nonzero(ours.diagonal()) > 5
        assert np.array_equal(ours.indptr, ref.indptr) and np.array_equal(ours.indices, ref.indices)
        diag = np.repeat(np.arange(a.shape[0]), np.diff(ours.indptr)) == ours.indices
        assert common.same_bits(ours.data[~diag], ref.data[~diag])
        assert np.array_equal(ours.data[diag] * np.float32(2), ref.data[diag]) and diag.sum() > 5
    else:                                                      # directed: the reference mirrors its upper triangle, we never add entries
        assert common.same_csr(sp.triu(ours, k=1), sp.triu(ref, k=1))
        lower = sp.tril(ours, k=-1).tocoo()
        assert all(a[j, i] != 0 for i, j in zip(lower.row, lower.col))          # every kept lower entry has a stored mirror


def test_the_mask_of_the_reference_is_written_but_ours_is_only_read(goldens):
    g = goldens.npz("g20_transforms")
    a = common.g20_graph(goldens, "symdiag48")
    mask = g["symdiag48|edge_mask"].copy()
    common.oracle_matrix(a, entry_keep=mask, symmetric_mask=True)
    assert np.array_equal(mask, g["symdiag48|edge_mask"])


@pytest.mark.parametrize("name", G20_GRAPHS)
def test_oracle_equals_scipy_submatrix(goldens, name):
    a = common.g20_graph(goldens, name)
    rng = np.random.RandomState(3)
    for share in (0.0, 0.1, 0.5, 1.0):
        m = rng.rand(a.shape[0]) < share
        id_map, n_out = common.mask_to_map(m)
        got = common.oracle_matrix(a, row_map=id_map, col_map=id_map, n_rows_out=n_out, n_cols_out=n_out)
        assert common.same_csr(got, a[m][:, m]), share
    rows, cols = rng.rand(a.shape[0]) < 0.6, rng.rand(a.shape[1]) < 0.4              # different row and column selections
    rmap, nr = common.mask_to_map(rows)
    cmap, nc = common.mask_to_map(cols)
    assert common.same_csr(common.oracle_matrix(a, row_map=rmap, col_map=cmap, n_rows_out=nr, n_cols_out=nc), a[rows][:, cols])


def test_hostile_map_values_count_as_dropped():
    a = common.zoo(n_rows=203, n_cols=211, long_row=150)
    rmap, nr = common.mask_to_map(np.arange(203) % 2 == 0)
    want = common.oracle_matrix(a, row_map=rmap, n_rows_out=nr)
    for bad in (-2, nr, np.iinfo(np.int32).max, np.iinfo(np.int32).min):
        hostile = rmap.copy()
        hostile[rmap < 0] = bad
        assert common.same_csr(common.oracle_matrix(a, row_map=hostile, n_rows_out=nr), want)


# ---- the random draws ------------------------------------------------------------------------------------------------------------------
def test_threshold_is_exact():
    from sgl_amd.transforms import drop_threshold
    assert drop_threshold(0.0) == 0
    assert drop_threshold(2.0 ** -60) == 16
    assert drop_threshold(0.5) == 1 << 63
    assert drop_threshold(1.0 - 2.0 ** -53) == (1 << 64) - (1 << 11)
    assert drop_threshold(1.0) == 1 << 64
    for p in (0.1, 0.3, 1 / 3, 0.999):
        t = drop_threshold(p)
        assert Fraction(t, 1 << 64) <= Fraction(p) < Fraction(t + 1, 1 << 64)
    for p in (-1e-9, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="Dropout probability has to be between 0 and 1!"):
            drop_threshold(p)


def test_both_directions_of_a_pair_get_one_decision():
    from sgl_amd.transforms import drop_threshold
    a = common.zoo(n_rows=301, n_cols=301, long_row=200, mirror=0.7)
    t = drop_threshold(0.5)
    keep, ri, cj = common.oracle_keep(a.indptr, a.indices, 301, drop_below=t, seed=9, symmetric=True)
    kept = set(zip(ri[keep].tolist(), cj[keep].tolist()))
    stored = set(zip(ri.tolist(), cj.tolist()))
    pairs = [(i, j) for (i, j) in stored if i != j and (j, i) in stored]
    assert len(pairs) > 1000
    assert all(((i, j) in kept) == ((j, i) in kept) for i, j in pairs)
    assert 0.4 < len(kept) / len(stored) < 0.6
    plain, _, _ = common.oracle_keep(a.indptr, a.indices, 301, drop_below=t, seed=9, symmetric=False)
    kept_plain = set(zip(ri[plain].tolist(), cj[plain].tolist()))
    assert any(((i, j) in kept_plain) != ((j, i) in kept_plain) for i, j in pairs)     # without `symmetric` the directions are independent


def test_dropped_share_of_the_draws():
    """10^5 pairs at p = 0.3: the dropped share within 5 sqrt(p (1 - p) / N) of p (5 standard deviations of a binomial share)"""
    from sgl_amd.transforms import drop_threshold
    n, p = 100_000, 0.3
    bound = 5 * np.sqrt(p * (1 - p) / n)
    rng = np.random.RandomState(1)
    i, j = rng.randint(0, 1 << 20, size=n), rng.randint(0, 1 << 20, size=n)
    for seed in (0, 1, 12345):
        for stream, a, b in ((common.EDGE_DROP_STREAM, np.minimum(i, j), np.maximum(i, j)), (common.NODE_DROP_STREAM, np.arange(n), np.zeros(n, dtype=np.int64))):
            dropped = (_hash4(seed, stream, a.astype(np.uint64), b.astype(np.uint64)) < np.uint64(drop_threshold(p))).mean()
            print(seed, stream, dropped, bound)
            assert abs(dropped - p) <= bound, (seed, stream, dropped)


def test_node_keep_mask_equals_the_numpy_mirror():
    from sgl_amd.transforms import drop_threshold, node_keep_mask
    n = 5000
    for seed, p in ((0, 0.5), (3, 0.3), ((1 << 64) - 5, 0.9), (1, 2.0 ** -60)):
        want = _hash4(seed, common.NODE_DROP_STREAM, np.arange(n, dtype=np.uint64), np.uint64(0)) >= np.uint64(drop_threshold(p))
        assert np.array_equal(node_keep_mask(n, p, seed, device="cpu").numpy(), want), (seed, p)
    assert not node_keep_mask(n, 1.0, 0, device="cpu").any()


# ---- the Python layer's argument checks (no device is reached) ----------------------------------------------------------------------
def test_error_messages_and_identity_of_the_python_layer(goldens):
    from sgl_amd import transforms as tr
    a = common.g20_graph(goldens, "sym64")
    for fn in (tr.random_drop_edges, tr.random_drop_nodes):
        for p in (-0.1, 1.5):
            with pytest.raises(ValueError, match="Dropout probability has to be between 0 and 1!"):
                fn(a, p=p)
    assert tr.random_drop_edges(a, p=0.0) is a                                       # p = 0: the input object
    from sgl_amd.io import DeviceAdjacency
    host = DeviceAdjacency(torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int32)),
                           torch.from_numpy(a.data.astype(np.float32)), a.shape)     # a container of CPU tensors: refused before any launch
    assert tr.random_drop_edges(host, p=0.0) is host
    sub, mask = tr.random_drop_nodes(host, p=0.0)
    assert sub.adj is host and mask.all() and mask.numel() == 64
    for bad in (np.ones(a.nnz + 1, dtype=bool), np.ones((a.nnz, 1), dtype=bool), torch.ones(a.nnz - 1, dtype=torch.bool)):
        for fn in (tr.drop_edges, tr.biased_drop_edges):
            with pytest.raises(ValueError, match="the shape of edge drop mask is wrong!"):
                fn(host, bad)
    for bad in (np.ones(65, dtype=bool), np.ones((64, 1), dtype=bool), [True] * 63):
        with pytest.raises(ValueError, match="the shape of node mask is wrong!"):
            tr.get_subgraph(host, bad)


def test_mask_features_modes():
    from sgl_amd import transforms as tr
    x = torch.arange(12, dtype=torch.float32).reshape(4, 3) + 1
    keep = x.clone()
    rows = torch.tensor([True, False, False, True])
    cols = torch.tensor([False, True, False])
    elem = (x % 2 == 0)
    assert torch.equal(tr.mask_features(x, rows), torch.where(rows[:, None], torch.zeros_like(x), x))
    assert torch.equal(tr.mask_features(x, cols, type=1), torch.where(cols[None, :], torch.zeros_like(x), x))
    assert torch.equal(tr.mask_features(x, elem, type=2), torch.where(elem, torch.zeros_like(x), x))
    assert torch.equal(x, keep)                                                      # a copy: x itself is never written
    with pytest.raises(ValueError, match="the choice of type is 0, 1, or 2!"):
        tr.mask_features(x, rows, type=3)
    for mask, kind in ((cols, 0), (rows, 1), (rows, 2)):
        with pytest.raises(ValueError, match="dimension does not match"):
            tr.mask_features(x, mask, type=kind)

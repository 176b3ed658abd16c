"""CPU-side checks of the edge split (csrc/sgl_edge_split.hip, tricks/link_prediction.py: has_edges, mask_test_edges): the two
exported symbols and their bindings, their error contract without a GPU -- a non-zero code and a message that names the entry, nothing
launched -- and the test oracle itself: check_split accepts what the REFERENCE's mask_test_edges returned (tests/golden/
g17_edge_split.npz), the sequential oracle passes the same checks strictly, and its draw counts stay under the default max_draws."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT

import edge_split_common as common
from sgl_amd import _lib

FIND, CANDIDATES = "sgl_csr_find", "sgl_edge_candidates"
G17_GRAPHS = ("sym64", "pl256", "dir40")
G17_NAMES = ("train_edges", "train_edges_false", "val_edges", "val_edges_false", "test_edges", "test_edges_false")


@pytest.mark.parametrize("name", [FIND, CANDIDATES])
def test_library_exports_the_symbols(name):
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, name), f"{name} is not exported by libsgl_hip.so"
    assert name in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 105


@pytest.mark.parametrize("name,count", [(FIND, 8), (CANDIDATES, 9)])
def test_header_and_binding_argument_counts_agree(name, count):
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sgl_hip.h"
    params = [p for p in m.group(1).split(",") if p.strip()]
    restype, argtypes = _lib.PROTOTYPES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == count, (len(argtypes), params)
    assert "d_rowptr" in m.group(1) and "d_edges" in m.group(1)


def test_public_names_are_exported():
    from sgl_amd import device as dev
    from sgl_amd import tricks
    from sgl_amd.tricks import link_prediction as lp
    for name in ("has_edges", "mask_test_edges", "EdgeSplit"):
        assert name in lp.__all__ and name in tricks.__all__ and hasattr(tricks, name)
    assert callable(dev.csr_find) and callable(dev.edge_candidates)
    assert lp.EdgeSplit._fields == ("adj_train",) + G17_NAMES                  # the reference's return order
    assert "mask_test_edges" in lp.nafs_link_prediction.__doc__


class Args:
    """valid calls on HOST memory that is never touched (a zero-length call returns before any launch; every bad call is refused
    before): a 4 x 4 matrix, room for 8 pairs.  off(p, k): the address k bytes behind p."""

    def __init__(self):
        self.rowptr = (ctypes.c_int64 * 5)()
        self.col = (ctypes.c_int32 * 8)()
        self.edges = (ctypes.c_int64 * 18)()
        self.out = (ctypes.c_int64 * 10)()
        p = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
        self.find = dict(rowptr=p(self.rowptr), col=p(self.col), n_rows=4, n_cols=4, edges=p(self.edges), q=0, pos=p(self.out))
        self.cand = dict(rowptr=p(self.rowptr), col=p(self.col), n=4, seed=7, first=0, count=0, edges=p(self.edges), key=p(self.out))

    @staticmethod
    def off(p, k):
        return ctypes.c_void_p(p.value + k)

    def call_find(self, **change):
        k = dict(self.find, **change)
        return _lib.lib().sgl_csr_find(k["rowptr"], k["col"], k["n_rows"], k["n_cols"], k["edges"], k["q"], k["pos"], None)

    def call_cand(self, **change):
        k = dict(self.cand, **change)
        return _lib.lib().sgl_edge_candidates(k["rowptr"], k["col"], k["n"], k["seed"], k["first"], k["count"], k["edges"], k["key"], None)


def refused(call, name, **change):
    rc = call(**change)
    msg = _lib.last_error()
    assert rc != 0, change
    assert msg and name in msg, (change, msg)


def test_csr_find_rejects_bad_arguments_without_a_gpu():
    a = Args()
    assert a.call_find() == 0, _lib.last_error()                                # Q = 0: nothing to do, no device needed
    assert a.call_find(edges=a.off(a.find["edges"], 8)) == 0, _lib.last_error()   # 8-byte alignment of the list is enough
    assert a.call_find(n_rows=0, n_cols=0) == 0, _lib.last_error()
    for q in (0, 5):                                                            # bad arguments are refused whatever Q is
        for key in ("rowptr", "col", "edges", "pos"):
            refused(a.call_find, FIND, q=q, **{key: None})
        refused(a.call_find, FIND, q=q, n_rows=-1)
        refused(a.call_find, FIND, q=q, n_cols=-1)
        refused(a.call_find, FIND, q=q, n_cols=1 << 31)                         # columns are int32
        refused(a.call_find, FIND, q=q, rowptr=a.off(a.find["rowptr"], 4))
        refused(a.call_find, FIND, q=q, col=a.off(a.find["col"], 2))
        refused(a.call_find, FIND, q=q, edges=a.off(a.find["edges"], 4))
        refused(a.call_find, FIND, q=q, pos=a.off(a.find["pos"], 4))
    refused(a.call_find, FIND, q=-1)


def test_edge_candidates_rejects_bad_arguments_without_a_gpu():
    a = Args()
    assert a.call_cand() == 0, _lib.last_error()                                # count = 0
    assert a.call_cand(first=1 << 40, seed=(1 << 64) - 1) == 0, _lib.last_error()
    assert a.call_cand(n=(1 << 31) - 1) == 0, _lib.last_error()
    assert a.call_cand(edges=a.off(a.cand["edges"], 8)) == 0, _lib.last_error()
    for count in (0, 5):
        for key in ("rowptr", "col", "edges", "key"):
            refused(a.call_cand, CANDIDATES, count=count, **{key: None})
        refused(a.call_cand, CANDIDATES, count=count, n=1 << 31)                # the key min * n + max must fit int64
        refused(a.call_cand, CANDIDATES, count=count, n=0)
        refused(a.call_cand, CANDIDATES, count=count, n=-3)
        refused(a.call_cand, CANDIDATES, count=count, first=-1)
        refused(a.call_cand, CANDIDATES, count=count, rowptr=a.off(a.cand["rowptr"], 4))
        refused(a.call_cand, CANDIDATES, count=count, col=a.off(a.cand["col"], 2))
        refused(a.call_cand, CANDIDATES, count=count, edges=a.off(a.cand["edges"], 4))
        refused(a.call_cand, CANDIDATES, count=count, key=a.off(a.cand["key"], 4))
    refused(a.call_cand, CANDIDATES, count=-1)
    refused(a.call_cand, CANDIDATES, first=(1 << 63) - 2, count=5)              # first + count overflows


def test_torch_hash_equals_the_numpy_mirror():
    """the shuffle's hash is computed with int64 torch arithmetic: the same 64 bits as synthetic._hash4, the same unsigned order"""
    from sgl_amd.synthetic import _hash4
    from sgl_amd.tricks import link_prediction as lp
    e = np.arange(3000, dtype=np.uint64)
    for seed in (0, 1, 2, (1 << 64) - 5):
        want = _hash4(seed, common.SHUFFLE_STREAM, e, 0)
        got = lp._hash4(seed, common.SHUFFLE_STREAM, torch.arange(3000, dtype=torch.int64), 0).numpy().view(np.uint64)
        assert np.array_equal(got, want), seed
        assert (want >> np.uint64(63)).any() and not (want >> np.uint64(63)).all()      # the unsigned order is really exercised
        assert np.array_equal(lp._shuffle_order(seed, 3000, "cpu").numpy(), np.argsort(want, kind="stable"))


# ---- the checker against the reference's own output, the oracle against the checker ---------------------------------------------------
def recorded(goldens, name):
    g = goldens.npz("g17_edge_split")
    n = goldens.graph(name).shape[0]
    adj_train = sp.csr_matrix((g[f"{name}|adj_train|data"], g[f"{name}|adj_train|indices"], g[f"{name}|adj_train|indptr"]), shape=(n, n))
    return (adj_train,) + tuple(g[f"{name}|{key}"] for key in G17_NAMES)


@pytest.mark.parametrize("name", G17_GRAPHS)
def test_check_split_accepts_what_the_reference_returned(goldens, name):
    adj = goldens.graph(name)
    common.check_split(adj, recorded(goldens, name), strict_val=False)


def test_check_split_notices_a_broken_split(goldens):
    adj = goldens.graph("sym64")
    good = recorded(goldens, "sym64")
    stored = sorted(common.stored_set(adj))
    for slot, change in ((2, lambda f: np.concatenate((f[:-1], f[:1]))),             # a negative pair twice
                         (6, lambda f: np.concatenate((f[:-1], good[2][:1, ::-1]))),   # a train negative, mirrored, among the test ones
                         (6, lambda f: np.concatenate((f[:-1], np.array([stored[0]])))),   # a stored pair
                         (6, lambda f: np.concatenate((f[:-1], np.array([[3, 3]])))),  # a self pair
                         (1, lambda p: p[:-1]),                                        # a train edge missing
                         (5, lambda p: np.concatenate((p[:-1], good[3][:1])))):        # a val edge among the test edges
        bad = list(good)
        bad[slot] = change(good[slot])
        with pytest.raises(AssertionError):
            common.check_split(adj, tuple(bad), strict_val=False)


def graphs_of_the_gpu_tests(goldens):
    return [(name, goldens.graph(name)) for name in ("sym64", "pl256", "pl2000", "dir40")] + [("weighted40", common.weighted40())]


def test_oracle_passes_the_strict_checks_and_has_the_reference_sizes(goldens):
    for name, adj in graphs_of_the_gpu_tests(goldens):
        for seed in (1, 2):
            out, _ = common.oracle_split(adj, seed)
            common.check_split(adj, out, strict_val=True)
            if name in G17_GRAPHS:
                ref = recorded(goldens, name)
                assert [len(x) for x in out[1:]] == [len(x) for x in ref[1:]], name
                assert out[0].nnz == ref[0].nnz
    out, _ = common.oracle_split(goldens.graph("pl256"), 1, negatives=("test",))
    common.check_split(goldens.graph("pl256"), out, negatives=("test",))


# need -> candidates drawn by the sequential loop, seeds 1 and 2 (computed on the CPU with the numpy mirror of the stream)
DRAWS = {"sym64": (156, 182, 183), "pl256": (915, 961, 956), "pl2000": (6818, 6861, 6857), "dir40": (71, 88, 82)}


def test_oracle_draw_counts_stay_under_the_default_max_draws(goldens):
    for name, adj in graphs_of_the_gpu_tests(goldens):
        for k, seed in enumerate((1, 2)):
            out, drawn = common.oracle_split(adj, seed)
            need = len(out[2]) + len(out[4]) + len(out[6])
            print(name, seed, need, drawn)
            assert need <= drawn <= 64 * need + 65536
            if name in DRAWS:
                assert (need, drawn) == (DRAWS[name][0], DRAWS[name][1 + k]), name
    adj = common.half_dense8()
    assert len(common.stored_set(adj)) == 28 and adj.shape == (8, 8)             # 14 of the 28 pairs, both orientations
    for seed in (1, 2, 3, 4, 5):                                                 # every admissible pair is needed: 69 .. 81 draws
        out, drawn = common.oracle_split(adj, seed)
        need = len(out[2]) + len(out[4]) + len(out[6])
        print("half_dense8", seed, need, drawn)
        assert need == 14 and drawn <= 64 * need + 65536
    assert len(common.stored_set(common.half_dense8(extra=True))) == 30

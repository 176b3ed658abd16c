"""CPU-side checks of the k-means path (csrc/sgl_kmeans.hip, tricks/clustering.py): the exported symbol and its binding, the error
contract of sgl_kmeans_assign_f32 without a GPU -- a non-zero code and a message that names the entry, nothing launched -- the three
clustering scores against the values the reference returned (tests/golden/g16_node_clustering.npz), and the inputs of the GPU kernel
tests: how many rows their float64 reference itself leaves out as near a tie."""
import ctypes
import os
import re

import numpy as np
import torch

from conftest import ROOT

from kmeans_common import MAX_LEFT_OUT, N_ROWS, cases, reference
from sgl_amd import _lib

NAME = "sgl_kmeans_assign_f32"


def test_library_exports_the_symbol():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, NAME), f"{NAME} is not exported by libsgl_hip.so"
    assert NAME in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 104


def test_header_and_binding_argument_counts_agree():
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared in include/sgl_hip.h"
    params = [p for p in m.group(1).split(",") if p.strip()]
    restype, argtypes = _lib.PROTOTYPES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 10, (len(argtypes), params)
    assert "d_centres" in m.group(1) and "d_mindist" in m.group(1) and "int64_t *d_labels" in m.group(1)


class Args:
    """a valid call on HOST memory that is never touched (n = 0 returns before any launch; every bad call is refused before): a
    [4, 8] matrix and two centres on pitches of 8"""

    def __init__(self):
        self.x = (ctypes.c_float * 64)()
        self.c = (ctypes.c_float * 16)()
        self.labels = (ctypes.c_int64 * 8)()
        self.dist = (ctypes.c_float * 8)()
        self.kw = dict(x=ctypes.cast(self.x, ctypes.c_void_p), ldx=8, n=0, d=8, c=ctypes.cast(self.c, ctypes.c_void_p), ldc=8, k=2,
                       labels=ctypes.cast(self.labels, ctypes.c_void_p), dist=ctypes.cast(self.dist, ctypes.c_void_p))

    def call(self, **change):
        k = dict(self.kw, **change)
        return _lib.lib().sgl_kmeans_assign_f32(k["x"], k["ldx"], k["n"], k["d"], k["c"], k["ldc"], k["k"], k["labels"], k["dist"], None)

    def shifted(self, name, by):
        return ctypes.c_void_p(self.kw[name].value + by)


def refused(args, **change):
    rc = args.call(**change)
    msg = _lib.last_error()
    assert rc != 0, change
    assert msg and NAME in msg, (change, msg)
    return rc


def test_entry_rejects_bad_arguments_without_a_gpu():
    a = Args()
    assert a.call() == 0, _lib.last_error()                           # n = 0: nothing to do, no device needed
    assert a.call(d=0) == 0, _lib.last_error()
    assert a.call(dist=None) == 0, _lib.last_error()                  # the distances are optional
    assert a.call(k=0) == 0, _lib.last_error()                        # no rows need no centre
    assert a.call(x=None, labels=None, dist=None) == 0, _lib.last_error()   # ... and no storage (an empty tensor's pointer is NULL)
    for n in (0, 5):                                                  # bad arguments are refused whatever n is
        refused(a, n=n, d=-1)
        refused(a, n=n, d=2 ** 31 - 1, ldx=2 ** 31, ldc=2 ** 31)
        refused(a, n=n, k=-1)
        refused(a, n=n, ldx=7)                                        # pitch < d
        refused(a, n=n, ldc=7)
        refused(a, n=n, x=a.shifted("x", 2))                          # not aligned to the element size
        refused(a, n=n, c=a.shifted("c", 2))
        refused(a, n=n, dist=a.shifted("dist", 2))
        refused(a, n=n, labels=a.shifted("labels", 4))
    refused(a, n=5, x=None)                                           # rows and columns, but no storage
    refused(a, n=5, c=None)
    refused(a, n=5, labels=None)
    refused(a, n=5, k=0)                                              # rows, but no centre
    refused(a, n=-1)


def test_clustering_scores_reproduce_the_recorded_reference_values(goldens):
    """both sides are float64 evaluations of the same expressions of one integer table: 1e-12"""
    from sgl_amd.tricks import clustering_scores
    g = goldens.npz("g16_node_clustering")
    for name in ("perfect", "noisy", "fewer"):
        true, pred, want = g[f"metrics|{name}|true"], g[f"metrics|{name}|pred"], g[f"metrics|{name}|scores"]
        for got in (clustering_scores(torch.from_numpy(true), torch.from_numpy(pred)), clustering_scores(true, pred.tolist())):
            print(name, got, want)
            assert all(isinstance(v, float) for v in got)
            assert np.abs(np.array(got) - want).max() <= 1e-12, (name, got, want)
    assert int(g["metrics|fewer|reference_raised"][0]) == 1 and g["metrics|fewer|scores"][0] == 0.0
    assert len(np.unique(g["metrics|fewer|pred"])) < len(np.unique(g["metrics|fewer|true"]))
    acc, nmi, adjscore = clustering_scores(g["metrics|perfect|true"], g["metrics|perfect|pred"])
    assert acc == 1.0 and adjscore == 1.0 and abs(nmi - 1.0) <= 2.0 ** -50
    assert not np.array_equal(g["metrics|perfect|true"], g["metrics|perfect|pred"])      # the match really is permuted


def test_kernel_test_inputs_leave_few_rows_near_a_tie():
    """the label comparison of test_gpu_kmeans.py skips the rows its float64 reference calls near a tie: at most 1 % of a case"""
    worst = (0.0, (0, 0))
    for d, k in cases():
        share = float(reference(d, k)[2].mean())
        worst = max(worst, (share, (d, k)))
        assert share <= MAX_LEFT_OUT, (d, k, share)
    print("largest left-out share", worst, "of", N_ROWS, "rows")

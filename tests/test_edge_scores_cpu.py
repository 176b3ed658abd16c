"""CPU-side checks of the edge-score path (csrc/sgl_edge.hip, tricks/link_prediction.py): the exported symbol and its binding, the
error contract of sgl_edge_dot_f32 without a GPU -- a non-zero code and a message that names the entry, nothing launched -- and the
ranking metrics against the values sklearn gave the reference (tests/golden/g14_link_prediction.npz)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from sgl_amd import _lib

NAME = "sgl_edge_dot_f32"


def test_library_exports_the_symbol():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, NAME), f"{NAME} is not exported by libsgl_hip.so"
    assert NAME in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 103


def test_header_and_binding_argument_counts_agree():
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared in include/sgl_hip.h"
    params = [p for p in m.group(1).split(",") if p.strip()]
    restype, argtypes = _lib.PROTOTYPES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 11, (len(argtypes), params)
    assert "d_edges" in m.group(1) and "int64_t" in m.group(1)


class Args:
    """a valid call on HOST memory that is never touched (n_edges = 0 returns before any launch; every bad call is refused before):
    two [4, 8] matrices on a pitch of 8"""

    def __init__(self):
        self.a = (ctypes.c_float * 64)()
        self.b = (ctypes.c_float * 64)()
        self.e = (ctypes.c_int64 * 16)()
        self.o = (ctypes.c_float * 16)()
        self.kw = dict(a=ctypes.cast(self.a, ctypes.c_void_p), lda=8, n_a=4, b=ctypes.cast(self.b, ctypes.c_void_p), ldb=8, n_b=4,
                       e=ctypes.cast(self.e, ctypes.c_void_p), n_edges=0, d=8, o=ctypes.cast(self.o, ctypes.c_void_p))

    def call(self, **change):
        k = dict(self.kw, **change)
        return _lib.lib().sgl_edge_dot_f32(k["a"], k["lda"], k["n_a"], k["b"], k["ldb"], k["n_b"], k["e"], k["n_edges"], k["d"], k["o"], None)


def refused(args, **change):
    rc = args.call(**change)
    msg = _lib.last_error()
    assert rc != 0, change
    assert msg and NAME in msg, (change, msg)
    return rc


def test_entry_rejects_bad_arguments_without_a_gpu():
    a = Args()
    assert a.call() == 0, _lib.last_error()                           # n_edges = 0: nothing to do, no device needed
    assert a.call(d=0) == 0, _lib.last_error()
    assert a.call(a=a.kw["b"]) == 0, _lib.last_error()                # B may be A
    for n_edges in (0, 5):                                            # bad arguments are refused whatever n_edges is
        refused(a, n_edges=n_edges, a=None)
        refused(a, n_edges=n_edges, b=None)
        refused(a, n_edges=n_edges, e=None)
        refused(a, n_edges=n_edges, o=None)
        refused(a, n_edges=n_edges, d=-1)
        refused(a, n_edges=n_edges, lda=7)                            # ld < d
        refused(a, n_edges=n_edges, ldb=7)
    refused(a, n_edges=-1)


# ---- the ranking metrics against what sklearn returned to the reference ---------------------------------------------------------------
def recorded_sets(goldens):
    g = goldens.npz("g14_link_prediction")
    n_pos, n_neg = len(g["pos_edges"]), len(g["neg_edges"])
    labels = np.concatenate((np.ones(n_pos, np.float32), np.zeros(n_neg, np.float32)))
    for key in sorted(k[:-len("|metrics")] for k in g if k.startswith("lp|") and k.endswith("|metrics")):
        yield key, g[key + "|probs"], labels, g[key + "|metrics"]
    for name in ("ties", "distinct"):
        key = f"metrics|{name}"
        yield key, g[key + "|probs"], g[key + "|labels"], g[key + "|metrics"]


def test_binary_ranking_metrics_reproduce_the_recorded_sklearn_values(goldens):
    """both sides are float64 evaluations of one rational number: within n_scores * 2^-52"""
    from sgl_amd.tricks import binary_ranking_metrics
    seen = 0
    for key, probs, labels, want in recorded_sets(goldens):
        roc_auc, avg_prec = binary_ranking_metrics(torch.from_numpy(probs), torch.from_numpy(labels))
        tol = len(probs) * 2.0 ** -52
        print(key, abs(roc_auc - want[0]), abs(avg_prec - want[1]), tol)
        assert isinstance(roc_auc, float) and isinstance(avg_prec, float)
        assert abs(roc_auc - want[0]) <= tol, (key, roc_auc, want[0])
        assert abs(avg_prec - want[1]) <= tol, (key, avg_prec, want[1])
        seen += 1
    assert seen == 4 * 4 + 2
    ties = goldens.npz("g14_link_prediction")["metrics|ties|probs"]
    assert (ties == 1.0).sum() > 20                                   # the saturated set really has its ties


def test_binary_ranking_metrics_raise_for_a_single_class():
    from sgl_amd.tricks import binary_ranking_metrics
    s = torch.tensor([0.1, 0.7, 0.7, 0.3])
    for labels in (torch.ones(4), torch.zeros(4)):
        with pytest.raises(ValueError):
            binary_ranking_metrics(s, labels)
    # by hand: groups {0.7: one of each}, {0.3: positive}, {0.1: negative} -> (FP, TP) = (1, 1), (1, 2), (2, 2)
    roc_auc, avg_prec = binary_ranking_metrics(s, torch.tensor([0., 1., 0., 1.]))
    assert roc_auc == 0.625 and abs(avg_prec - (0.25 + 1.0 / 3.0)) <= 2.0 ** -52

"""CPU-side checks of the trainable clustering path (csrc/sgl_cluster_loss.hip, tricks/clustering.py): the exported symbol and its
binding, the error contract of sgl_cluster_loss_grad_f32 without a GPU -- a non-zero code and a message that names the entry, nothing
launched -- the condition that the acceptance rule of the GPU tests puts on their inputs (a plain float32 numpy restatement passes it
on every case), the restatement against what the reference recorded (tests/golden/g19_node_clustering_train.npz), cluster_loss's label
rules and the best-of bookkeeping of node_clustering."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle
from cluster_loss_common import (cases, compiled_instances, inputs, parse_kernel_name, references, restated_step, rows_per_group,
                                 step_references, SHIFT)
from conftest import ROOT
from sgl_amd import _lib

NAME = "sgl_cluster_loss_grad_f32"


def test_library_exports_the_symbol():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, NAME), f"{NAME} is not exported by libsgl_hip.so"
    assert NAME in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 107
    from sgl_amd import tricks
    from sgl_amd.tricks import clustering as cl
    for name in ("cluster_loss", "clustering_train", "node_clustering", "NodeClusteringTrainResult"):
        assert name in cl.__all__ and name in tricks.__all__ and hasattr(tricks, name)


def test_header_and_binding_argument_counts_agree():
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    assert re.search(r"^ \*   " + NAME + r"\s", text, flags=re.M), "the entry is missing from the header's list of entry points"
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared in include/sgl_hip.h"
    params = [p for p in m.group(1).split(",") if p.strip()]
    restype, argtypes = _lib.PROTOTYPES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 13, (len(argtypes), params)
    assert "d_centres" in m.group(1) and "const int64_t *d_labels" in m.group(1) and "float w" in m.group(1) and "d_row_loss" in m.group(1)
    assert "sgl_cluster_loss.hip" in open(os.path.join(ROOT, "sgl_amd", "csrc", "build.py")).read()


class Args:
    """a valid call on HOST memory that is never touched (n = 0 returns before any launch; every bad call is refused before): a
    [4, 8] matrix and two centres on pitches of 8"""

    def __init__(self):
        self.x = (ctypes.c_float * 64)()
        self.c = (ctypes.c_float * 16)()
        self.dx = (ctypes.c_float * 64)()
        self.labels = (ctypes.c_int64 * 8)()
        self.loss = (ctypes.c_float * 8)()
        as_p = lambda a: ctypes.cast(a, ctypes.c_void_p)
        self.kw = dict(x=as_p(self.x), ldx=8, n=0, d=8, c=as_p(self.c), ldc=8, k=2, labels=as_p(self.labels), w=0.25, dx=as_p(self.dx),
                       lddx=8, loss=as_p(self.loss))

    def call(self, **change):
        k = dict(self.kw, **change)
        return _lib.lib().sgl_cluster_loss_grad_f32(k["x"], k["ldx"], k["n"], k["d"], k["c"], k["ldc"], k["k"], k["labels"], k["w"], k["dx"],
                                                    k["lddx"], k["loss"], None)

    def shifted(self, name, by):
        return ctypes.c_void_p(self.kw[name].value + by)


def refused(args, **change):
    rc = args.call(**change)
    msg = _lib.last_error()
    assert rc == 1001, (change, rc)                                   # SGL_ERR_INVALID
    assert msg and NAME in msg, (change, msg)


def test_entry_rejects_bad_arguments_without_a_gpu():
    a = Args()
    assert a.call() == 0, _lib.last_error()                           # n = 0: nothing to do, no device needed
    assert a.call(d=0) == 0, _lib.last_error()
    assert a.call(dx=None) == 0, _lib.last_error()                    # either output is optional
    assert a.call(loss=None) == 0, _lib.last_error()
    assert a.call(x=None, labels=None, dx=None, loss=None) == 0, _lib.last_error()   # no rows need no storage (an empty tensor's pointer is NULL)
    refused(a, n=5, dx=None, loss=None)                               # ... but with rows not both
    for n in (0, 5):                                                  # bad arguments are refused whatever n is
        refused(a, n=n, k=0)                                          # k < 1, with or without rows
        refused(a, n=n, k=-1)
        refused(a, n=n, d=-1)
        refused(a, n=n, d=2 ** 31 - 1, ldx=2 ** 31, ldc=2 ** 31, lddx=2 ** 31)
        refused(a, n=n, ldx=7)                                        # pitch < d
        refused(a, n=n, ldc=7)
        refused(a, n=n, lddx=7)
        refused(a, n=n, c=None)
        refused(a, n=n, x=a.shifted("x", 2))                          # not aligned to the element size
        refused(a, n=n, c=a.shifted("c", 2))
        refused(a, n=n, dx=a.shifted("dx", 2))
        refused(a, n=n, loss=a.shifted("loss", 2))
        refused(a, n=n, labels=a.shifted("labels", 4))
    refused(a, n=5, x=None)                                           # rows and columns, but no storage
    refused(a, n=5, labels=None)
    refused(a, n=-1)


# ---- the condition the acceptance rule puts on the inputs ----------------------------------------------------------------------------------
def check_restatement(d, k, shift, worst):
    x, c, y = inputs(d, k, shift)
    refs = references(d, k, shift)
    loss, dx = restated_step(x, c, y)
    for i, (what, got) in enumerate((("loss", loss), ("dX", dx))):
        rep = oracle.truth_report(got, refs["ref32"][i], refs["truth"][i], cond=refs["cond"][i])
        assert rep["ok"] and np.isfinite(np.asarray(got)).all(), (d, k, shift, what, rep)
        worst[what] = max(worst[what], (rep["err_got"] / rep["cond_bound_max"], (d, k, shift)))


def test_float32_restatement_passes_the_acceptance_rule_on_every_gpu_case():
    """pins the condition: the reference's float32 error, doubled (or the floor), admits a straightforward float32 evaluation of the
    same formula on every (d, k) of test_gpu_cluster_loss.py, zero-distance centres included"""
    worst = {"loss": (0.0, None), "dX": (0.0, None)}
    for d, k in cases():
        check_restatement(d, k, 0.0, worst)
    print("largest error over the largest bound", worst)


def test_float32_restatement_passes_on_the_shifted_inputs():
    worst = {"loss": (0.0, None), "dX": (0.0, None)}
    for d, k in ((7, 2), (100, 47), (147, 7), (600, 64)):
        check_restatement(d, k, SHIFT, worst)
    print("largest error over the largest bound", worst)


def test_references_have_zero_distances_and_a_finite_gradient_there():
    x, c, y = inputs(100, 47)
    hit = (x[:, None, :] == c[None, :3, :]).all(-1)
    assert hit.sum() == 3
    refs = references(100, 47)
    assert np.isfinite(refs["ref32"][1]).all() and np.isfinite(refs["truth"][1]).all()
    # k = 1: every label is 0 and l_i = D_i
    x, c, y = inputs(12, 1)
    assert (y == 0).all()
    dist = np.sqrt(((x.astype(np.float64) - c[0].astype(np.float64)) ** 2).sum(1))
    assert abs(references(12, 1)["truth"][0] - dist.mean()) <= 1e-12 * dist.mean()


def test_instance_rule_restated():
    want = compiled_instances()
    assert len(want) == 16 and all(u == rows_per_group(v, c) for _, v, c, u in want if c)
    assert parse_kernel_name("void (anonymous namespace)::cluster_loss_kernel<32, 4, 1, 4>(float const*, long)") == (32, 4, 1, 4)
    assert parse_kernel_name("_ZN12_GLOBAL__N_119cluster_loss_kernelILi64ELi1ELi32ELi1EEEvPKflliS2_liiilPKlffPflS5_") == (64, 1, 32, 1)
    assert parse_kernel_name("_ZN12_GLOBAL__N_126cluster_loss_stream_kernelILi4EEEvPKflliS2_liPKlffPflS5_") == (64, 4, 0, 1)
    assert parse_kernel_name("void (anonymous namespace)::kmeans_assign_kernel<32, 4, 1, 4>(float const*)") is None


# ---- the reference fixture ------------------------------------------------------------------------------------------------------------------
def test_restated_step_reproduces_the_reference_fixture(goldens):
    """G19 (a): the float64 restatement against the reference's own float64 loss and gradient, the float32 one under the rule the GPU
    kernel is held to; and the CPU references of the GPU tests (step_references) ARE the recorded numbers"""
    g = goldens.npz("g19_node_clustering_train")
    z, c, y = g["step|z"], g["step|centres"], g["step|labels"]
    assert (z[7] == c[0]).all()                                       # the zero distance
    loss64, dx64 = restated_step(z.astype(np.float64), c, y)
    assert abs(loss64 - float(g["step|loss64"])) <= 1e-14 and np.allclose(dx64, g["step|grad64"], rtol=0, atol=1e-16)
    refs = step_references(z, c, y)
    assert abs(refs["truth"][0] - float(g["step|loss64"])) <= 1e-14 and np.allclose(refs["truth"][1], g["step|grad64"], rtol=0, atol=1e-16)
    loss, dx = restated_step(z, c, y)
    for what, got, ref32, truth, cond in (("loss", loss, g["step|loss"], g["step|loss64"], refs["cond"][0]),
                                          ("dX", dx, g["step|grad"], g["step|grad64"], refs["cond"][1])):
        rep = oracle.truth_report(got, ref32, truth, cond=cond)
        print(what, rep)
        assert rep["ok"], (what, rep)


# ---- cluster_loss's labels ------------------------------------------------------------------------------------------------------------------
def test_label_wrapping_and_index_error():
    from sgl_amd.tricks.clustering import _device_labels
    k, n = 5, 6
    for form in (np.array([0, 4, -1, -5, 2, 3]), torch.tensor([0, 4, -1, -5, 2, 3]), [0, 4, -1, -5, 2, 3], np.array([0, 4, -1, -5, 2, 3], dtype=np.int32)):
        got = _device_labels(form, k, n, torch.device("cpu"), True)
        assert got.dtype == torch.int64 and got.is_contiguous() and got.tolist() == [0, 4, 4, 0, 2, 3]
    assert _device_labels(np.array([0, 9, -7, 1, 1, 1]), k, n, torch.device("cpu"), False).tolist() == [0, 9, -7, 1, 1, 1]
    for bad in ([0, 5, 0, 0, 0, 0], [0, -6, 0, 0, 0, 0], [2 ** 40, 0, 0, 0, 0, 0]):
        for form in (np.array(bad), torch.tensor(bad)):
            with pytest.raises(IndexError):
                _device_labels(form, k, n, torch.device("cpu"), True)
    with pytest.raises(ValueError):
        _device_labels([0, 1], k, n, torch.device("cpu"), True)
    with pytest.raises(TypeError):
        _device_labels(np.zeros(n, dtype=np.float32), k, n, torch.device("cpu"), True)
    from sgl_amd.tricks import cluster_loss
    with pytest.raises(ValueError):
        cluster_loss(torch.zeros(2, 2), [0, 0], torch.zeros(1, 2), reduction="max")
    with pytest.raises(TypeError):
        cluster_loss(torch.zeros(2, 2), [0, 0], torch.zeros(1, 2))    # not a CUDA matrix


# ---- the bookkeeping of the task -----------------------------------------------------------------------------------------------------------
class StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def preprocess(self, adj, x):
        self.calls.append(("preprocess", adj, x))

    def model_forward(self, idx, device):
        self.calls.append(("forward", len(idx), self.training))
        return torch.zeros(len(idx), 2)

    def postprocess(self, adj, out):
        self.calls.append(("postprocess", adj))
        return out + 1.0


def test_node_clustering_keeps_the_best_of_each_score(monkeypatch):
    from sgl_amd.tricks import clustering as cl
    per_epoch = [(0.5, 0.5, 0.2, 0.1), (0.4, 0.7, 0.1, 0.1), (0.3, 0.6, 0.3, 0.0), (0.2, 0.7, 0.3, 0.1)]      # loss, acc, nmi, adjscore
    final = (0.1, 0.25, 0.4)
    seeds = []

    def train(model, idx, y, optimizer, n_clusters, n_init=20, seed=None, device="cuda"):
        assert isinstance(optimizer, torch.optim.Adam) and n_clusters == 3 and n_init == 7 and len(idx) == 6
        assert optimizer.defaults["lr"] == 0.5 and optimizer.defaults["weight_decay"] == 0.25
        seeds.append(seed)
        return per_epoch[len(seeds) - 1]

    def fake_kmeans(x, k, n_init=20, seed=None, **kw):
        assert k == 3 and n_init == 7 and bool((x == 1.0).all())      # the postprocessed output
        seeds.append(("final", seed))
        return cl.KMeansResult(torch.zeros(len(x), dtype=torch.int64), None, 0.0, 1)

    monkeypatch.setattr(cl, "clustering_train", train)
    monkeypatch.setattr(cl, "kmeans", fake_kmeans)
    monkeypatch.setattr(cl, "clustering_scores", lambda y, pred: final)
    model = StubModel()
    res = cl.node_clustering(model, "adj", "x", np.array([0, 1, 2, 2, 1, 0]), epochs=4, lr=0.5, weight_decay=0.25, n_init=7, seed=10, device="cpu")
    assert isinstance(res, cl.NodeClusteringTrainResult)
    assert (res.acc, res.nmi, res.adjscore) == (0.7, 0.3, 0.4)        # strictly greater wins; the final step counts too
    assert seeds == [10, 11, 12, 13, ("final", 14)]
    assert [h["epoch"] for h in res.history] == [0, 1, 2, 3, "post"] and [h["loss"] for h in res.history[:-1]] == [0.5, 0.4, 0.3, 0.2]
    assert res.history[-1] == dict(epoch="post", acc=0.1, nmi=0.25, adjscore=0.4) and res.history[1]["acc"] == 0.7
    assert model.calls == [("preprocess", "adj", "x"), ("forward", 6, False), ("postprocess", "adj")]
    # bests start at 0: scores that never exceed it leave it
    seeds.clear()
    per_epoch[:] = [(1.0, 0.0, -0.5, -0.25)] * 4
    monkeypatch.setattr(cl, "clustering_scores", lambda y, pred: (0.0, 0.0, -1.0))
    res = cl.node_clustering(StubModel(), "adj", "x", [0, 1, 2, 2, 1, 0], epochs=4, lr=0.5, weight_decay=0.25, n_init=7, seed=10, device="cpu")
    assert (res.acc, res.nmi, res.adjscore) == (0.0, 0.0, 0.0)

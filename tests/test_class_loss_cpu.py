"""CPU-side checks of the node-classification path (csrc/sgl_class_loss.hip, tricks/classification.py): the exported symbol and its
binding, the error contract of sgl_class_loss_grad_f32 without a GPU -- a non-zero code and a message that names the entry, nothing
launched -- the condition that the acceptance rule of the GPU tests puts on their inputs (a plain float32 numpy restatement passes it
at every width), the arg-max cases, the restated instance rule against the instances the source compiles, the restatement against
what the reference recorded (tests/golden/g21_node_classification.npz), argument validation of the Python functions, the batch order
and the bookkeeping of the task."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import oracle
from class_loss_common import (CHUNKS, IGNORE, WIDTHS, argmax_cases, compiled_instances, inputs, instance_for, parse_kernel_name,
                               reference_pred, references, restated_rows, restated_step, rows_per_group, step_references, unique_maximum, weight)
from conftest import ROOT
from sgl_amd import _lib

NAME = "sgl_class_loss_grad_f32"
PUBLIC = ("cross_entropy", "loge_cross_entropy", "predict", "accuracy", "train", "mini_batch_train", "evaluate", "mini_batch_evaluate",
          "node_classification", "NodeClassificationResult")


def test_library_exports_the_symbol():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, NAME), f"{NAME} is not exported by libsgl_hip.so"
    assert NAME in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 109
    from sgl_amd import device as dev
    from sgl_amd import tricks
    from sgl_amd.tricks import classification as cl
    assert callable(dev.class_loss_grad)
    for name in PUBLIC:
        assert name in cl.__all__ and name in tricks.__all__ and hasattr(tricks, name)


def test_header_and_binding_argument_counts_agree():
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    assert re.search(r"^ \*   " + NAME + r"\s", text, flags=re.M), "the entry is missing from the header's list of entry points"
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared in include/sgl_hip.h"
    params = [p for p in m.group(1).split(",") if p.strip()]
    restype, argtypes = _lib.PROTOTYPES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 11, (len(argtypes), params)
    assert "const int64_t *d_labels" in m.group(1) and "float w" in m.group(1) and "d_row_loss" in m.group(1) and "int64_t *d_pred" in m.group(1)
    assert "sgl_class_loss.hip" in open(os.path.join(ROOT, "sgl_amd", "csrc", "build.py")).read()


class Args:
    """a valid call on HOST memory that is never touched (n = 0 returns before any launch; every bad call is refused before): a
    [4, 8] matrix on a pitch of 8"""

    def __init__(self):
        self.z = (ctypes.c_float * 64)()
        self.dz = (ctypes.c_float * 64)()
        self.labels = (ctypes.c_int64 * 8)()
        self.loss = (ctypes.c_float * 8)()
        self.pred = (ctypes.c_int64 * 8)()
        as_p = lambda a: ctypes.cast(a, ctypes.c_void_p)
        self.kw = dict(z=as_p(self.z), ldz=8, n=0, c=8, labels=as_p(self.labels), w=0.25, dz=as_p(self.dz), lddz=8, loss=as_p(self.loss),
                       pred=as_p(self.pred))

    def call(self, **change):
        k = dict(self.kw, **change)
        return _lib.lib().sgl_class_loss_grad_f32(k["z"], k["ldz"], k["n"], k["c"], k["labels"], k["w"], k["dz"], k["lddz"], k["loss"], k["pred"],
                                                  None)

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
    for gone in ("dz", "loss", "pred"):                               # every output is optional
        assert a.call(**{gone: None}) == 0, _lib.last_error()
    assert a.call(z=None, labels=None, dz=None, loss=None, pred=None) == 0, _lib.last_error()   # no rows need no storage
    refused(a, n=5, dz=None, loss=None, pred=None)                    # ... but with rows not all three
    for n in (0, 5):                                                  # bad arguments are refused whatever n is
        refused(a, n=n, c=0)                                          # c < 1, with or without rows
        refused(a, n=n, c=-1)
        refused(a, n=n, c=2 ** 31, ldz=2 ** 31, lddz=2 ** 31)
        refused(a, n=n, ldz=7)                                        # pitch < c
        refused(a, n=n, lddz=7)
        refused(a, n=n, z=a.shifted("z", 2))                          # not aligned to the element size
        refused(a, n=n, dz=a.shifted("dz", 2))
        refused(a, n=n, loss=a.shifted("loss", 2))
        refused(a, n=n, labels=a.shifted("labels", 4))
        refused(a, n=n, pred=a.shifted("pred", 4))
    assert a.call(lddz=7, dz=None) == 0, _lib.last_error()            # the pitch of an output that is not asked for is not looked at
    refused(a, n=5, z=None)                                           # rows, but no storage
    refused(a, n=5, labels=None)                                      # the labels may be missing only for pred alone
    refused(a, n=5, labels=None, dz=None)
    refused(a, n=-1)


# ---- the condition the acceptance rule puts on the inputs ----------------------------------------------------------------------------------
def test_float32_restatement_passes_the_acceptance_rule_at_every_gpu_width():
    """pins the condition: the reference's float32 error, doubled (or the floor), admits a straightforward float32 evaluation of the
    same formula at every width of test_gpu_class_loss.py, the rows of magnitude 1e4 included"""
    worst = {"loss": (0.0, 0), "dZ": (0.0, 0)}
    for c in WIDTHS:
        z, y = inputs(c)
        assert (y[::17] == IGNORE).all() and np.abs(z).max() > 9e3
        refs = references(c)
        loss, dz = restated_step(z, y)
        for i, (what, got) in enumerate((("loss", loss), ("dZ", dz))):
            rep = oracle.truth_report(got, refs["ref32"][i], refs["truth"][i], cond=refs["cond"][i])
            assert rep["ok"] and np.isfinite(np.asarray(got)).all(), (c, what, rep)
            worst[what] = max(worst[what], (rep["err_got"] / rep["cond_bound_max"], c))
        ignored = y == IGNORE
        assert (refs["ref32"][1][ignored] == 0).all() and (dz[ignored] == 0).all()
    print("largest error over the largest bound", worst)


def test_argmax_cases_and_unique_maxima():
    """the random rows of the value tests have a unique float32 maximum (so the arg-max is a property of the input, not of an order);
    the constructed rows hold ties and NaNs, where the lowest index and the first NaN win -- torch's CPU max, restated"""
    for c in WIDTHS:
        z, _ = inputs(c)
        unique = unique_maximum(z)
        assert unique.sum() >= (len(z) // 2 if c > 1 else len(z)), c   # (rows around 1e4 with a spread of 0.1 do tie in float32)
        assert (restated_rows(z, np.zeros(len(z), np.int64), 1.0)[2][unique] == z.argmax(1)[unique]).all()
    for c in (3, 7, 47, 172, 1030, 2500):
        z = argmax_cases(c)
        want = reference_pred(z)
        for i in range(0, len(z), 8):
            assert (z[i] == np.nanmax(z[i])).sum() == 2 and want[i] == np.flatnonzero(z[i] == z[i].max())[0]
            assert (z[i + 1] == np.nanmax(z[i + 1])).sum() == 3 and want[i + 1] == np.flatnonzero(z[i + 1] == z[i + 1].max())[0]
            assert np.isnan(z[i + 2]).sum() == 1 and want[i + 2] == np.flatnonzero(np.isnan(z[i + 2]))[0]
            assert np.isnan(z[i + 3]).sum() == 2 and want[i + 3] == np.flatnonzero(np.isnan(z[i + 3]))[0]


def test_instance_rule_against_the_compiled_instances():
    want = compiled_instances()
    assert len(want) == 16
    # the chunk counts of the 64-lane instances stand once, in sgl_common.h: the rule (sgl::slice_instance, sgl_core.cpp) and the
    # dispatch (with_slice_instance, sgl_rows.h) of the entry point both read that list
    src = open(os.path.join(ROOT, "sgl_amd", "csrc", "sgl_class_loss.hip")).read()
    common = open(os.path.join(ROOT, "sgl_amd", "csrc", "sgl_common.h")).read()
    lists = re.findall(r"using ClassLossSlices = SliceFamily<Chunks<([\d, ]+)>, Chunks<([\d, ]+)>>;", common)
    assert len(lists) == 1 and {vec: tuple(int(v) for v in chs.split(",")) for vec, chs in zip((4, 1), lists[0])} == CHUNKS
    assert "sgl::slice_instance(c, vec, sgl::ClassLossSlices::chunks(vec))" in src and "with_one_of<" not in src
    assert "with_slice_instance<sgl::ClassLossSlices>(" in src and "launch_rows<L, V, C>" in src and "class_loss_stream_kernel<V>" in src
    core = open(os.path.join(ROOT, "sgl_amd", "csrc", "sgl_core.cpp")).read()
    assert "SliceInstance slice_instance(int64_t width, int vec, ChunkList compiled)" in core
    assert (max(CHUNKS[4]), max(CHUNKS[1])) == (4, 16)                                # the largest CH per lane size
    assert {instance_for(c, 4) for c in WIDTHS} == {i for i in want if i[1] == 4}, "the widths do not reach every 16-byte instance"
    assert {instance_for(c, 1) for c in WIDTHS} == {i for i in want if i[1] == 1}, "the widths do not reach every 4-byte instance"
    assert instance_for(47, 4) == (16, 4, 1) and instance_for(172, 4) == (64, 4, 1) and instance_for(3, 1) == (8, 1, 1)
    assert instance_for(1024, 4) == (64, 4, 4) and instance_for(1025, 4) == (64, 4, 0)
    assert instance_for(1024, 1) == (64, 1, 16) and instance_for(1025, 1) == (64, 1, 0)
    assert parse_kernel_name("void (anonymous namespace)::class_loss_kernel<16, 4, 1, 4>(float const*, long)") == (16, 4, 1)
    assert parse_kernel_name("_ZN12_GLOBAL__N_117class_loss_kernelILi64ELi1ELi16ELi1EEEvPKflliPKlfPflS5_Pll") == (64, 1, 16)
    assert parse_kernel_name("_ZN12_GLOBAL__N_124class_loss_stream_kernelILi4EEEvPKflliPKlfPflS5_Pl") == (64, 4, 0)
    assert parse_kernel_name("void (anonymous namespace)::cluster_loss_kernel<32, 4, 1, 4>(float const*)") is None
    assert [rows_per_group(v, k) for v, k in ((1, 1), (1, 2), (1, 4), (1, 8), (1, 16), (4, 1), (4, 2), (4, 4))] == [8, 8, 4, 2, 1, 4, 2, 1]
    with pytest.raises(ValueError):
        parse_kernel_name("void (anonymous namespace)::class_loss_kernel<16, 4, 1, 8>(float const*, long)")


# ---- the reference fixture ------------------------------------------------------------------------------------------------------------------
def test_restated_step_reproduces_the_reference_fixture(goldens):
    """G21 (a): the float64 restatement against the reference's own float64 loss and gradient, the float32 one under the rule the GPU
    kernel is held to; LogeCrossEntropy as the scalar transform of the mean loss; and the CPU references of the GPU tests
    (step_references) ARE the recorded numbers"""
    g = goldens.npz("g21_node_classification")
    z, y = g["step|z"], g["step|labels"]
    assert (y == IGNORE).sum() == 6
    loss64, dz64 = restated_step(z.astype(np.float64), y)
    assert abs(loss64 - float(g["step|ce|loss64"])) <= 1e-11 and np.allclose(dz64, g["step|ce|grad64"], rtol=0, atol=1e-15)
    refs = step_references(z, y)
    assert refs["truth"][0] == float(g["step|ce|loss64"]) and np.array_equal(refs["truth"][1], g["step|ce|grad64"])
    assert np.array_equal(refs["ref32"][1], g["step|ce|grad"])
    loss, dz = restated_step(z, y)
    eps = 1.0 - math.log(2)
    chain = 1.0 / (eps + loss64)                                      # d loge / d ce, in float64
    for what, got, ref32, truth, cond in (("loss", loss, g["step|ce|loss"], g["step|ce|loss64"], refs["cond"][0]),
                                          ("dZ", dz, g["step|ce|grad"], g["step|ce|grad64"], refs["cond"][1]),
                                          ("loge", math.log(eps + loss) - math.log(eps), g["step|loge|loss"], g["step|loge|loss64"], refs["cond"][0] * chain),
                                          ("loge dZ", dz * np.float32(1.0 / (eps + loss)), g["step|loge|grad"], g["step|loge|grad64"], refs["cond"][1] * chain)):
        rep = oracle.truth_report(got, ref32, truth, cond=cond)
        print(what, rep)
        assert rep["ok"], (what, rep)
    assert abs((math.log(eps + loss64) - math.log(eps)) - float(g["step|loge|loss64"])) <= 1e-12
    assert np.allclose(dz64 * chain, g["step|loge|grad64"], rtol=0, atol=1e-15)


def test_accuracy_fixture_restated(goldens):
    g = goldens.npz("g21_node_classification")
    z, y = g["acc|z"], g["acc|labels"]
    assert ((z == z.max(1, keepdims=True)).sum(1) > 1).sum() >= 20    # exact ties
    pred = restated_rows(z, y, 1.0)[2]
    assert np.array_equal(pred, g["acc|pred"]) and float((pred == y).sum() / len(y)) == float(g["acc|value"])


def test_loop_fixture_restated(goldens):
    """G21 (c): the first recorded loss IS the restated mean loss of the stub model's initial output, and the first recorded training
    accuracy the restated arg-max's (float64: no tolerance beyond its rounding)"""
    g = goldens.npz("g21_node_classification")
    x, y, idx = g["loop|x"].astype(np.float64), g["loop|y"], g["loop|train_idx"]
    out = x[idx] @ g["loop|state|lin.weight"].astype(np.float64).T + g["loop|state|lin.bias"].astype(np.float64)
    loss, _ = restated_step(out, y[idx])
    for key in ("full|ce|history64", "task|history64"):
        assert abs(loss - g[key][0, 0]) <= 1e-12 and float((out.argmax(1) == y[idx]).mean()) == g[key][0, 1]
    eps = 1.0 - math.log(2)
    assert abs(math.log(eps + loss) - math.log(eps) - g["full|loge|history64"][0, 0]) <= 1e-12
    first = g["loop|train_batches"][0]
    out = x[first] @ g["loop|state|lin.weight"].astype(np.float64).T + g["loop|state|lin.bias"].astype(np.float64)
    assert restated_step(out, y[first])[0] <= g["mini|ce|history64"][0, 0] * 4                    # (the mean of four positive batch losses)
    assert sorted(g["loop|train_batches"].reshape(-1).tolist()) == idx.tolist()
    assert np.array_equal(g["task|best"], [g["task|history"][:, 2].max(), g["task|history"][g["task|history"][:, 2].argmax(), 3]])


# ---- the Python functions: what needs no launch -------------------------------------------------------------------------------------------
def test_argument_validation():
    from sgl_amd import device as dev
    from sgl_amd.tricks import accuracy, cross_entropy, loge_cross_entropy, predict, train
    from sgl_amd.tricks.classification import _class_labels
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError):
        cross_entropy(z, [0, 1, 2, 0], reduction="max")
    with pytest.raises(TypeError):
        cross_entropy(z, [0, 1, 2, 0], fused=True)                    # not a CUDA matrix
    with pytest.raises(TypeError):
        cross_entropy(z.to(torch.bfloat16), [0, 1, 2, 0], fused=True)
    with pytest.raises(TypeError):
        cross_entropy(torch.zeros(4), [0, 1, 2, 0])
    with pytest.raises(TypeError):
        cross_entropy(z, torch.zeros(4, 3), fused=False)              # probability targets
    with pytest.raises(ValueError):
        cross_entropy(z, [0, 1], fused=False)
    with pytest.raises(ValueError):
        loge_cross_entropy(z, [0, 1, 2, 0], reduction="sum", fused=False)
    for bad in ([0, 3, 0, 0], [0, -1, 0, 0], [2 ** 40, 0, 0, 0]):
        for form in (np.array(bad), torch.tensor(bad), bad):
            with pytest.raises(IndexError):
                cross_entropy(z, form, fused=False)
    y, live = _class_labels(np.array([0, 2, -100, 1], dtype=np.int32), 3, 4, torch.device("cpu"), -100, True)
    assert y.dtype == torch.int64 and y.tolist() == [0, 2, -1, 1] and live == 3
    y, live = _class_labels([0, 2, 5, 1], 3, 4, torch.device("cpu"), 1, False)                     # nothing checked: out of range = ignored
    assert y.tolist() == [0, 2, -1, -1] and torch.is_tensor(live) and int(live) == 2
    with pytest.raises(TypeError):
        predict(z)                                                    # the launch takes CUDA matrices; accuracy scores a host matrix on the host
    assert accuracy(torch.tensor([[0., 1.], [1., 1.], [2., 1.]]), [1, 0, 1]) == 2 / 3
    with pytest.raises(TypeError):
        dev.class_loss_grad(z, None, 1.0, pred=True)                  # not a CUDA matrix
    with pytest.raises(ValueError):
        train(None, [0], None, "cpu", None, loss_fn="hinge")
    with pytest.raises(TypeError):
        train(None, [0], None, "cpu", None, loss_fn=3)


def test_unfused_route_is_torch_and_takes_the_same_labels():
    from sgl_amd.tricks import cross_entropy, loge_cross_entropy
    z_h, y_h = inputs(7)
    refs = references(7)
    z = torch.from_numpy(z_h).requires_grad_(True)
    loss, pred = cross_entropy(z, y_h, fused=False, return_pred=True)
    loss.backward()
    assert float(loss.detach()) == refs["ref32"][0] and np.array_equal(z.grad.numpy(), refs["ref32"][1])
    assert np.array_equal(pred.numpy(), reference_pred(z_h))
    y2 = np.where(y_h == 3, 1000, y_h)                                # check=False: out of range means ignored, as -100 does
    a = cross_entropy(torch.from_numpy(z_h), y2, fused=False, check=False)
    b = cross_entropy(torch.from_numpy(z_h), np.where(y_h == 3, IGNORE, y_h), fused=False)
    c = cross_entropy(torch.from_numpy(z_h), np.where(y_h == IGNORE, 3, y_h), fused=False, ignore_index=3)
    assert float(a) == float(b) == float(c)
    total = cross_entropy(torch.from_numpy(z_h), y_h, fused=False, reduction="sum")
    assert abs(float(total) * weight(y_h, 7) - refs["truth"][0]) <= 1e-5 * abs(refs["truth"][0])
    eps = 1.0 - math.log(2)
    assert abs(float(loge_cross_entropy(torch.from_numpy(z_h), y_h, fused=False)) - (math.log(eps + refs["truth"][0]) - math.log(eps))) <= 1e-5
    assert math.isnan(float(cross_entropy(torch.zeros(3, 2), [IGNORE] * 3, fused=False)))


def test_batch_order_is_determined_by_the_seed():
    from sgl_amd.tricks import epoch_batches
    idx = np.arange(100, 203)
    a, b, c = (epoch_batches(idx, 16, seed=s) for s in (5, 5, 6))
    assert [len(t) for t in a] == [16] * 6 + [7]
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and not all(torch.equal(p, q) for p, q in zip(a, c))
    assert sorted(torch.cat(a).tolist()) == idx.tolist() and sorted(torch.cat(c).tolist()) == idx.tolist()
    kept = epoch_batches(range(10), 4)
    assert [t.tolist() for t in kept] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    with pytest.raises(ValueError):
        epoch_batches(idx, 0)


# ---- the loops and the bookkeeping of the task, on the host with the unfused loss ------------------------------------------------------------
class Stub(torch.nn.Module):
    def __init__(self, x, w, b, post=None):
        super().__init__()
        self.lin = torch.nn.Linear(w.shape[1], w.shape[0])
        self.load_state_dict({"lin.weight": torch.from_numpy(w), "lin.bias": torch.from_numpy(b)})
        self.x, self.post, self.calls = torch.from_numpy(x), post, []

    def preprocess(self, adj, x):
        self.calls.append("preprocess")

    def model_forward(self, idx, device):
        from sgl_amd.tricks.classification import _as_index
        return self.lin(self.x[_as_index(idx, "cpu")])

    def postprocess(self, adj, out):
        self.calls.append("postprocess")
        return out if self.post is None else torch.from_numpy(self.post) @ out


def host_loss(out, y):
    return torch.nn.functional.cross_entropy(out, y)


def test_loops_follow_the_reference_on_the_host(goldens):
    """G21 (c) and (d) through train / evaluate / their mini-batch forms / node_classification with a callable loss on host tensors:
    the arithmetic around the kernel -- the mean of the batch losses, the correct count over len(train_idx), Adam, best-of -- is the
    reference's (the GPU test runs the same fixture through the kernel)"""
    from sgl_amd.tricks import node_classification
    g = goldens.npz("g21_node_classification")
    w, b = g["loop|state|lin.weight"], g["loop|state|lin.bias"]
    tr, va, te = g["loop|train_idx"], g["loop|val_idx"], g["loop|test_idx"]
    kw = dict(epochs=int(g["loop|epochs"]), lr=float(g["loop|lr"]), weight_decay=0.0, loss_fn=host_loss, device="cpu")
    model = Stub(g["loop|x"], w, b, g["task|post"])
    res = node_classification(model, "adj", None, g["loop|y"], tr, va, te, **kw)
    hist = np.array([[h["loss"], h["acc_train"], h["acc_val"], h["acc_test"]] for h in res.history[:-1]])
    assert np.array_equal(hist[:, 1:], g["task|history"][:, 1:]) and np.abs(hist[:, 0] - g["task|history64"][:, 0]).max() <= 1e-5
    assert res.history[-1] == dict(epoch="post", acc_val=g["task|post|acc"][0], acc_test=g["task|post|acc"][1])
    assert [res.best_val, res.best_test] == g["task|best"].tolist() and model.calls == ["preprocess", "postprocess"]
    assert np.abs(model.lin.weight.detach().numpy() - g["full|ce|final64|lin.weight"]).max() <= 1e-4
    model = Stub(g["loop|x"], w, b)
    res = node_classification(model, "adj", None, g["loop|y"], tr, va, te, eval_batch_size=int(g["loop|eval_batch"]),
                              batches={"train": [r for r in g["loop|train_batches"]]}, **kw)
    hist = np.array([[h["loss"], h["acc_train"], h["acc_val"], h["acc_test"]] for h in res.history[:-1]])
    assert np.array_equal(hist[:, 1:], g["mini|ce|history"][:, 1:]) and np.abs(hist[:, 0] - g["mini|ce|history64"][:, 0]).max() <= 1e-5
    assert np.abs(model.lin.weight.detach().numpy() - g["mini|ce|final64|lin.weight"]).max() <= 1e-4
    with pytest.raises(ValueError):
        node_classification(model, "adj", None, g["loop|y"], tr, va, te, train_batch_size=16, **kw)   # no eval_batch_size
    with pytest.raises(ValueError):
        node_classification(model, "adj", None, g["loop|y"], tr, va, te, batches={"valid": []}, **kw)


def test_node_classification_keeps_the_test_accuracy_of_the_best_validation(monkeypatch):
    from sgl_amd.tricks import classification as cl
    per_epoch = [((0.9, 0.5), (0.5, 0.7)), ((0.8, 0.6), (0.6, 0.1)), ((0.7, 0.6), (0.6, 0.9)), ((0.6, 0.7), (0.4, 1.0))]
    calls = []

    def train(model, idx, y, device, optimizer, loss_fn):
        assert isinstance(optimizer, torch.optim.Adam) and optimizer.defaults["lr"] == 0.5 and optimizer.defaults["weight_decay"] == 0.25
        calls.append("train")
        return per_epoch[len(calls) // 2][0]

    def evaluate(model, val_idx, test_idx, y, device):
        calls.append("eval")
        return per_epoch[len(calls) // 2 - 1][1]

    monkeypatch.setattr(cl, "train", train)
    monkeypatch.setattr(cl, "evaluate", evaluate)
    x = np.zeros((6, 2), dtype=np.float32)
    x[:, 0] = [1, 1, 1, -1, -1, -1]                                   # the stub predicts class 0 for rows 0 .. 2, class 1 for the rest
    w, b = np.array([[1, 0], [-1, 0]], dtype=np.float32), np.zeros(2, dtype=np.float32)
    y = [0, 0, 1, 1, 1, 0]
    res = cl.node_classification(Stub(x, w, b), "adj", None, y, [0], [0, 1, 2, 3], [2, 3, 4, 5], epochs=4, lr=0.5, weight_decay=0.25, device="cpu")
    # validation 0.5, 0.6, 0.6 (not strictly greater: its 0.9 is NOT taken), 0.4; post: val 3 / 4 > 0.6 takes test 2 / 4
    assert res.history[-1] == dict(epoch="post", acc_val=0.75, acc_test=0.5) and (res.best_val, res.best_test) == (0.75, 0.5)
    calls.clear()
    res = cl.node_classification(Stub(x, w, b), "adj", None, y, [0], [2, 5], [2, 3, 4, 5], epochs=4, lr=0.5, weight_decay=0.25, device="cpu")
    assert res.history[-1]["acc_val"] == 0.0 and (res.best_val, res.best_test) == (0.6, 0.1)
    assert [h["epoch"] for h in res.history] == [0, 1, 2, 3, "post"] and res.history[1] == dict(epoch=1, loss=0.8, acc_train=0.6, acc_val=0.6, acc_test=0.1)

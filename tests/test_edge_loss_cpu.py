"""CPU-side checks of the fused edge loss (csrc/sgl_edge_loss.hip, tricks/link_prediction.py: EdgePlan): the exported symbol and its
binding, the error contract of sgl_edge_loss_grad_f32 without a GPU, EdgePlan's tables on CPU tensors against a restatement with
loops, and the restated formulas against what the reference recorded (tests/golden/g18_gae_link_prediction.npz) -- which pins the
restatement the GPU tests lean on to the reference."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle
from conftest import ROOT
from edge_loss_common import HUB_EDGES, LABELS, hub_edges, loss_and_coef, plan_tables, restated_step, step_references
from edge_scores_common import EDGES, N_ROWS

from sgl_amd import _lib
from sgl_amd import device as dev

NAME = "sgl_edge_loss_grad_f32"


def test_library_exports_the_symbol():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, NAME), f"{NAME} is not exported by libsgl_hip.so"
    assert NAME in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 106
    from sgl_amd import tricks
    from sgl_amd.tricks import link_prediction as lp
    for name in ("EdgePlan", "edge_bce_loss", "edge_predict_train", "edge_predict_eval", "gae_link_prediction"):
        assert name in lp.__all__ and name in tricks.__all__ and hasattr(tricks, name)


def test_header_and_binding_argument_counts_agree():
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared in include/sgl_hip.h"
    params = [p for p in m.group(1).split(",") if p.strip()]
    restype, argtypes = _lib.PROTOTYPES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 25, (len(argtypes), params)
    assert "d_pieces" in m.group(1) and "d_inc_edge" in m.group(1)
    assert "sgl_edge_loss.hip" in open(os.path.join(ROOT, "sgl_amd", "csrc", "build.py")).read()


class Args:
    """a valid call on HOST memory that is never touched (n_pieces = 0 returns before any launch; every bad call is refused before)"""

    def __init__(self):
        self.keep = [(ctypes.c_float * 64)() for _ in range(6)] + [(ctypes.c_int64 * 64)() for _ in range(4)]

        def p(i):
            base = ctypes.addressof(self.keep[i])
            return ctypes.c_void_p((base + 31) // 32 * 32)
        self.kw = dict(z=p(0), ldz=8, n=4, d=8, pieces=p(6), n_pieces=0, other=p(7), edge=p(8), n_inc=4, labels=p(1), given=None, n_edges=2,
                       mode=0, w=0.5, dz=p(2), lddz=8, partial=p(3), ldp=8, n_partial=0, fold=p(9), n_fold=0, score=p(4), coef=p(5), loss=None)

    def call(self, **change):
        k = dict(self.kw, **change)
        return _lib.lib().sgl_edge_loss_grad_f32(k["z"], k["ldz"], k["n"], k["d"], k["pieces"], k["n_pieces"], k["other"], k["edge"], k["n_inc"],
                                                 k["labels"], k["given"], k["n_edges"], k["mode"], k["w"], k["dz"], k["lddz"], k["partial"],
                                                 k["ldp"], k["n_partial"], k["fold"], k["n_fold"], k["score"], k["coef"], k["loss"], None)


def refused(args, **change):
    rc = args.call(**change)
    msg = _lib.last_error()
    assert rc != 0, change
    assert msg and NAME in msg, (change, msg)


def test_entry_rejects_bad_arguments_without_a_gpu():
    a = Args()
    assert a.call() == 0, _lib.last_error()                           # no pieces: nothing to do, no device needed
    assert a.call(d=0) == 0, _lib.last_error()
    assert a.call(mode=1) == 0, _lib.last_error()
    assert a.call(mode=2, given=a.kw["labels"], score=None, coef=None) == 0, _lib.last_error()
    for n_pieces in (0, 3):                                           # bad arguments are refused whatever n_pieces is
        refused(a, n_pieces=n_pieces, z=None)
        refused(a, n_pieces=n_pieces, dz=None)
        refused(a, n_pieces=n_pieces, labels=None)
        refused(a, n_pieces=n_pieces, other=None)
        refused(a, n_pieces=n_pieces, mode=3)
        refused(a, n_pieces=n_pieces, mode=2)                         # GIVEN without coefficients (and with score / coef outputs)
        refused(a, n_pieces=n_pieces, mode=2, given=a.kw["labels"])   # GIVEN has no score / coef output
        refused(a, n_pieces=n_pieces, ldz=7)
        refused(a, n_pieces=n_pieces, lddz=7)
        refused(a, n_pieces=n_pieces, n_inc=5)                        # not twice the edges
        refused(a, n_pieces=n_pieces, d=-1)
        refused(a, n_pieces=n_pieces, n_fold=1)                       # more cut rows than partial rows
    refused(a, n_pieces=3, pieces=None)
    refused(a, n_pieces=-1)


# ---- the plan's tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_piece", [1, 8, None], ids=["piece1", "piece8", "default"])
@pytest.mark.parametrize("which", ["edges", "hub"])
def test_edge_plan_tables_on_cpu_tensors(which, max_piece):
    from sgl_amd.tricks import EdgePlan
    edges, labels = (EDGES, LABELS) if which == "edges" else (hub_edges(), LABELS[:HUB_EDGES])
    want = plan_tables(edges, N_ROWS, max_piece or dev.EDGE_LOSS_MAX_PIECE)
    for form in (torch.from_numpy(edges), edges, (edges[:, 0], edges[:, 1])):
        plan = EdgePlan(form, torch.from_numpy(labels), N_ROWS, max_piece=max_piece, device="cpu")
        got = (plan.inc_ptr, plan.inc_other, plan.inc_edge, plan.pieces, plan.fold)
        for g, w, dt in zip(got, want, (torch.int64, torch.int32, torch.int64, torch.int64, torch.int64)):
            assert g.dtype == dt and g.is_contiguous()
            assert np.array_equal(g.numpy(), w), (which, max_piece)
        assert plan.n_partial == want[5] and plan.n_pieces == len(want[3]) and plan.n_edges == len(edges) and plan.n == N_ROWS
        assert plan.edges.min() >= 0 and torch.equal(plan.labels, torch.from_numpy(labels))
        assert plan.piece_loss.shape == (plan.n_pieces,) and plan.coef.shape == plan.score.shape == (len(edges),)
    if which == "hub" and max_piece == 8:
        of_hub = plan.pieces[plan.pieces[:, 0] == 5]
        assert len(of_hub) == 38 and int(plan.fold[plan.fold[:, 0] == 5][0, 2]) == 38            # 301 incidences: 37 x 8 + 5
        isolated = plan.pieces[plan.pieces[:, 0] >= 200]
        assert len(isolated) == N_ROWS - 200 and bool((isolated[:, 1] == isolated[:, 2]).all()) and bool((isolated[:, 3] == -1).all())


def test_edge_plan_from_pos_neg_and_its_checks():
    from sgl_amd.tricks import EdgePlan
    plan = EdgePlan.from_pos_neg(EDGES[:600], EDGES[600:], N_ROWS, device="cpu")
    assert torch.equal(plan.labels, torch.cat((torch.ones(600), torch.zeros(400))))
    assert np.array_equal(plan.edges.numpy(), np.where(EDGES < 0, EDGES + N_ROWS, EDGES))
    empty = EdgePlan(np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.float32), 5, device="cpu")
    assert empty.n_edges == 0 and empty.n_pieces == 5 and empty.n_partial == 0
    for bad in ([[0, N_ROWS]], [[-N_ROWS - 1, 0]], [[2 ** 40, 1]]):
        for form in (np.array(bad), torch.tensor(bad)):
            with pytest.raises(IndexError):
                EdgePlan(form, [1.0], N_ROWS, device="cpu")
    with pytest.raises(ValueError):
        EdgePlan(EDGES, LABELS[:-1], N_ROWS, device="cpu")
    with pytest.raises(ValueError):
        EdgePlan(EDGES[:, :1], LABELS, N_ROWS, device="cpu")
    with pytest.raises(TypeError):
        EdgePlan(EDGES.astype(np.float32), LABELS, N_ROWS, device="cpu")
    with pytest.raises(ValueError):
        EdgePlan(EDGES, LABELS, N_ROWS, max_piece=-1, device="cpu")


# ---- the formulas ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sigmoid", "none"])
def test_restated_formulas_are_finite_and_match_float64(mode):
    s = np.array([0.0, 20.0, -20.0, 100.0, -100.0, 3e38, -3e38], dtype=np.float32)
    for y in (0.0, 1.0, 0.25):
        L, c = loss_and_coef(s, np.full(len(s), y, dtype=np.float32), 1.0, mode)
        assert L.dtype == np.float32 and np.isfinite(L).all() and np.isfinite(c).all(), (mode, y, L, c)
        # against torch's own float64 evaluation of the reference's expression, where that is finite; it forms x + max(-x, 0) + log(...), so
        # at |x| = 100 it carries an absolute error of a few 100 x 2^-53 itself: 1e-12 is the floor below which it says nothing
        t = torch.from_numpy(s[:5]).double().requires_grad_(True)
        pred = torch.sigmoid(t) if mode == "sigmoid" else t
        ref = torch.nn.functional.binary_cross_entropy_with_logits(pred, torch.full((5,), y, dtype=torch.float64), reduction="none")
        ref.sum().backward()
        assert np.allclose(L[:5], ref.detach().numpy(), rtol=4 * 2.0 ** -24, atol=1e-12), (mode, y, L[:5], ref)
        assert np.allclose(c[:5], t.grad.numpy(), rtol=16 * 2.0 ** -24, atol=1e-12), (mode, y, c[:5], t.grad)


@pytest.mark.parametrize("mode", ["sigmoid", "none"])
def test_torch_formulas_of_the_default_path_have_the_reference_gradient_at_zero(mode):
    """the loss and coefficient the unfused path of edge_bce_loss forms in torch (link_prediction._bce_terms) against autograd of the
    reference's expression, at logits of exactly 0 among others: c = sigma(s) - y there, not a subgradient of max / abs.  float64
    against float64: a few roundings relative, and absolutely what torch's own x + max(-x, 0) + log(...) carries at |x| = 30 (a few
    30 x 2^-53: 1e-13 is the floor below which it says nothing).  The float32 evaluation against the numpy restatement: differences of
    quantities of size <= 1 (sigma - y), so a few float32 roundings of 1"""
    from sgl_amd.tricks.link_prediction import _bce_terms
    s = torch.tensor([0.0, 0.0, 0.0, -0.0, 1.5, -2.0, 30.0, -30.0], dtype=torch.float64, requires_grad=True)
    y = torch.tensor([1.0, 0.0, 0.25, 1.0, 0.3, 1.0, 1.0, 0.0], dtype=torch.float64)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(torch.sigmoid(s) if mode == "sigmoid" else s, y, reduction="none")
    ref.sum().backward()
    L, c = _bce_terms(s.detach(), y, mode)
    assert torch.allclose(L, ref.detach(), rtol=8 * 2.0 ** -52, atol=1e-13), (L, ref)
    assert torch.allclose(c, s.grad, rtol=8 * 2.0 ** -52, atol=1e-13), (c, s.grad)
    if mode == "none":
        assert c[0] == -0.5 and c[1] == 0.5 and c[2] == 0.25 and c[3] == -0.5
    L32, c32 = _bce_terms(s.detach().float(), y.float(), mode)
    want = loss_and_coef(s.detach().float().numpy(), y.float().numpy(), 1.0, mode)
    assert np.allclose(L32.numpy(), want[0], rtol=4 * 2.0 ** -24, atol=0) and np.allclose(c32.numpy(), want[1], rtol=0, atol=4 * 2.0 ** -24)


@pytest.mark.parametrize("mode,key", [("sigmoid", "train"), ("none", "train_logits")])
def test_restated_step_reproduces_the_reference_fixture(goldens, mode, key):
    """the float32 restatement is held to the tolerance the GPU kernel is held to: at most twice the reference's own float32 error
    against its float64 run; and the CPU references of the GPU tests (step_references) ARE the recorded numbers"""
    g = goldens.npz("g18_gae_link_prediction")
    z = g["z"]
    edges = np.concatenate((g["pos_edges"], g["neg_edges"]))
    labels = np.concatenate((np.ones(len(g["pos_edges"]), np.float32), np.zeros(len(g["neg_edges"]), np.float32)))
    refs = step_references(z, edges, labels, mode)
    assert abs(refs["truth"][0] - float(g[key + "|loss64"])) <= 4 * 2.0 ** -52 and np.allclose(refs["truth"][1], g[key + "|grad64"], rtol=0, atol=2.0 ** -60)
    loss, dz = restated_step(z, edges, labels, mode)
    for what, got, ref32, truth, cond in (("loss", loss, g[key + "|loss"], g[key + "|loss64"], refs["cond"][0]),
                                          ("dZ", dz, g[key + "|grad"], g[key + "|grad64"], refs["cond"][1])):
        rep = oracle.truth_report(got, ref32, truth, cond=cond)
        print(mode, what, rep)
        assert rep["ok"], (mode, what, rep)
    loss64, dz64 = restated_step(z.astype(np.float64), edges, labels, mode)
    assert abs(loss64 - float(g[key + "|loss64"])) <= 1e-14 and np.allclose(dz64, g[key + "|grad64"], rtol=0, atol=1e-16)

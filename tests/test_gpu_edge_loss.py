"""The fused edge loss (csrc/sgl_edge_loss.hip), EdgePlan, its wrappers and the trainable link-prediction task on a real MI355X: run
with `-m gpu`.

Loss and dZ are compared with the reference's own expression, torch.mm(Z, Z.t())[e0, e1] -> sigmoid -> binary_cross_entropy_with_logits
under CPU autograd, in float32 and in float64 (the truth), through oracle.truth_report -- at most twice as far from the truth as the
reference's float32 result, with the condition-aware floor; no tolerance is chosen in this file.  Bit-for-bit claims use torch.equal.
Every launch runs under torch.profiler: the kernel instances seen must be the ones the restated selection rule (edge_loss_common)
announces, and all of them together exactly the compiled ones."""
import numpy as np
import pytest
import torch

import oracle
from edge_loss_common import (HUB_EDGES, HUB_NODE, LABELS, WIDTHS, compiled_instances, expected_instance, hub_edges, parse_kernel_name,
                              references, step_references)
from edge_scores_common import EDGES, N_EDGES, N_ROWS, gradient_references, host_matrix
from inputs import hash_matrix
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.tricks import (EdgePlan, EdgeSplit, binary_ranking_metrics, edge_bce_loss, edge_predict_eval, edge_predict_train, edge_scores,
                            gae_link_prediction)

pytestmark = pytest.mark.gpu

PIECES = (None, 8, 1)
BIT_WIDTHS = (7, 100, 147, 600)
POISONS = (float("nan"), 1e30)


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


class Trace:
    """Runs launches under torch.profiler and checks, at exit, that the edge_loss_grad_kernel instances that really ran are, in order,
    the ones `expect()` announced; every other kernel is ignored.  A profiler that reports no kernel names fails the comparison."""

    def __init__(self):
        self.expected, self.seen = [], set()

    def expect(self, label, z, mode, times=1):
        self.expected += [(label, expected_instance(z, mode))] * times

    def __enter__(self):
        from torch.profiler import ProfilerActivity, profile
        self.prof = profile(activities=[ProfilerActivity.CUDA])
        self.prof.__enter__()
        return self

    def __exit__(self, et, ev, tb):
        torch.cuda.synchronize()
        self.prof.__exit__(et, ev, tb)
        if et is not None:
            return False
        from torch.autograd import DeviceType
        evs = sorted((e for e in self.prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
        got = [p for p in (parse_kernel_name(e.name) for e in evs) if p is not None]
        assert len(got) == len(self.expected), (len(got), len(self.expected), len(evs), got[:3], self.expected[:3])
        wrong = [(i, lab, g, w) for i, (g, (lab, w)) in enumerate(zip(got, self.expected)) if g != w]
        assert not wrong, (len(wrong), wrong[:8])
        self.seen |= set(got)
        return False


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def padded(x, cuda, fill=0.0):
    """x in a dev.alloc_rows buffer whose pad columns d .. pitch hold `fill` (inside the row's own pitch: never out of bounds)"""
    n, d = x.shape
    t = dev.alloc_rows(n, d, cuda, zero_pad=False)
    dev.padded_parent(t).fill_(fill)
    t.copy_(torch.from_numpy(x))
    return t


def odd_view(x, cuda, fill=1e30):
    """x as columns 1 .. 1 + d of a wider matrix full of `fill`: rows that are only 4-byte aligned, the one-float-per-lane path"""
    n, d = x.shape
    wide = torch.full((n, d + 5), fill, dtype=torch.float32, device=cuda)
    v = wide[:, 1:1 + d]
    v.copy_(torch.from_numpy(x))
    assert v.data_ptr() % 16 != 0
    return v


LAYOUTS = {"padded": padded, "odd_view": odd_view}
_PLANS = {}


def plan_for(cuda, which="edges", max_piece=None):
    key = (which, max_piece)
    if key not in _PLANS:
        edges, labels = (EDGES, LABELS) if which == "edges" else (hub_edges(), LABELS[:HUB_EDGES])
        _PLANS[key] = EdgePlan(edges, labels, N_ROWS, max_piece=max_piece, device=cuda)
    return _PLANS[key]


def step(tr, label, z, plan, mode, layout="padded", given=None, outputs=True):
    """one launch of the low-level call into a NaN-filled dZ of the given layout: (loss, dZ, score, coef)"""
    n, d = z.shape
    dz = LAYOUTS[layout](np.full((n, d), np.nan, dtype=np.float32), z.device, fill=7.0)
    e = plan.n_edges
    score = torch.full((e,), 7.0, device=z.device) if (outputs and mode != "given") else None
    coef = torch.full((e,), 7.0, device=z.device) if (outputs and mode != "given") else None
    tr.expect(label, z, mode)
    w = 1.0 / e
    assert dev.edge_loss_grad(z, plan, mode, w=w, given=given, dz=dz, score=score, coef=coef) is dz
    loss = None if mode == "given" else float(plan.piece_loss.double().sum() * w)
    return loss, dz, score, coef


def same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


def check_truth(bad, label, loss, dz, refs):
    dz = dz.cpu().numpy()
    if not (np.isfinite(dz).all() and np.isfinite(loss)):
        bad.append((label, "not finite"))
        return
    for what, got, k in (("loss", loss, 0), ("dZ", dz, 1)):
        rep = oracle.truth_report(got, refs["ref32"][k], refs["truth"][k], cond=refs["cond"][k])
        if not rep["ok"]:
            bad.append((label, what, rep))


# ---- values, in every compiled instance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_values_in_every_instance(cuda, layout):
    bad = []
    with Trace() as tr:
        for d in WIDTHS:
            z = LAYOUTS[layout](host_matrix(d), cuda)
            assert expected_instance(z, "sigmoid")[1] == (4 if layout == "padded" else 1)
            for mode in ("sigmoid", "none"):
                refs = references(d, mode)
                for mp in PIECES:
                    label = (layout, d, mode, mp)
                    loss, dz, _, coef = step(tr, label, z, plan_for(cuda, max_piece=mp), mode, layout)
                    check_truth(bad, label, loss, dz, refs)
            # the coefficients read back through the GIVEN mode: the same sums, bit for bit (and every GIVEN instance runs)
            _, again, _, _ = step(tr, (layout, d, "given"), z, plan_for(cuda, max_piece=1), "given", layout, given=coef)
            if not same(again, dz):
                bad.append((layout, d, "GIVEN mode differs from the fused dZ"))
    print(f"\n[edge_loss {layout}] {len(WIDTHS)} widths, instances seen: {sorted(tr.seen)}")
    assert not bad, (len(bad), bad[:6])
    vec = 4 if layout == "padded" else 1
    want = {i for i in compiled_instances() if i[1] == vec}
    assert tr.seen == want, sorted(want ^ tr.seen)


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_bits(cuda, layout, monkeypatch):
    edges = torch.from_numpy(EDGES).to(cuda)
    other = "odd_view" if layout == "padded" else "padded"
    bad = []
    with Trace() as tr:
        for d in BIT_WIDTHS:
            z = LAYOUTS[layout](host_matrix(d), cuda)
            logits = dev.edge_dot(z, z, edges)
            for mode in ("sigmoid", "none"):
                base = {}
                for mp in PIECES:
                    plan = plan_for(cuda, max_piece=mp)
                    loss, dz, score, coef = step(tr, d, z, plan, mode, layout)
                    base[mp] = (loss, dz, coef)
                    if not same(score, logits):
                        bad.append((d, mode, mp, "score is not edge_dot's"))
                    loss2, dz2, score2, coef2 = step(tr, d, z, plan, mode, other)
                    if not (loss2 == loss and same(dz2, dz) and same(score2, score) and same(coef2, coef)):
                        bad.append((d, mode, mp, "a second run, into a dZ of the other layout, differs"))
                    _, dz3, _, _ = step(tr, d, z, plan, "given", layout, given=coef)
                    if not same(dz3, dz):
                        bad.append((d, mode, mp, "coef through the GIVEN mode does not reproduce dZ"))
                    if not same(coef, base[None][2]):
                        bad.append((d, mode, mp, "the coefficients depend on max_piece"))
                # the public path, fused: the same loss and, through autograd with an upstream factor of 1, the same dZ
                zg = z.detach().requires_grad_(True)
                plan = plan_for(cuda, max_piece=8)
                tr.expect(d, z, mode)
                loss_t, scores = edge_bce_loss(zg, plan, activation=mode, return_scores=True, fused=True)
                loss_t.backward()
                want = np.float32(base[8][0])
                if not (float(loss_t.detach()) == float(want) and same(scores, logits) and same(zg.grad, base[8][1])):
                    bad.append((d, mode, "edge_bce_loss differs from the low-level call", float(loss_t.detach()), float(want)))
                # plan reuse without fusing: the same logits, loss and gradient to rounding
                zu = z.detach().requires_grad_(True)
                tr.expect(d, z, "given")
                loss_u, scores_u = edge_bce_loss(zu, plan, activation=mode, return_scores=True, fused=False)
                loss_u.backward()
                if not (same(scores_u, logits) and abs(float(loss_u.detach()) - base[8][0]) <= 8 * 2.0 ** -24 * abs(base[8][0])):
                    bad.append((d, mode, "unfused path", float(loss_u.detach()), base[8][0]))
                check_truth(bad, (d, mode, "unfused"), float(loss_u.detach()), zu.grad, references(d, mode))
                # the piece table split over several launches of 100 pieces (the fold of the cut rows runs with the last)
                monkeypatch.setattr(dev, "EDGE_DOT_MAX_EDGES", 100)
                n_calls = -(-plan.n_pieces // 100)
                loss4, dz4, _, _ = step(tr, d, z, plan, mode, layout)
                tr.expect(d, z, mode, times=n_calls - 1)
                monkeypatch.undo()
                if not (n_calls > 1 and loss4 == base[8][0] and same(dz4, base[8][1])):
                    bad.append((d, mode, "split piece table", n_calls))
                # without grad: edge_dot and the formulas in torch -- the same logits; the loss is a mean of NON-NEGATIVE float32 terms, each
                # within a few roundings of the kernel's (exp and log1p to 1 - 2 ulp on both sides, three additions): 8 x 2^-24 relative
                with torch.no_grad():
                    loss5, scores5 = edge_bce_loss(z, plan, activation=mode, return_scores=True)
                if not (same(scores5, logits) and abs(float(loss5) - base[8][0]) <= 8 * 2.0 ** -24 * abs(base[8][0])):
                    bad.append((d, mode, "no-grad path", float(loss5), base[8][0]))
    assert not bad, bad


# ---- a hub, isolated nodes, hostile pads, saturated scores ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sigmoid", "none"])
def test_hub_list_and_isolated_nodes(cuda, mode):
    plan = plan_for(cuda, "hub", 8)
    of_hub = plan.pieces[plan.pieces[:, 0] == HUB_NODE]
    assert of_hub.shape[0] == 38 and plan.n_partial == 38                                  # 301 incidences in pieces of 8
    bad = []
    with Trace() as tr:
        for d in (7, 100, 147, 600):
            refs = references(d, mode, "hub")
            for layout in LAYOUTS:
                z = LAYOUTS[layout](host_matrix(d), cuda)
                loss, dz, _, _ = step(tr, d, z, plan, mode, layout)
                check_truth(bad, (d, layout), loss, dz, refs)
                if not bool((dz[200:] == 0).all()):                                      # the dZ buffer was full of NaN
                    bad.append((d, layout, "an isolated node's row is not exact zeros"))
                loss1, dz1, _, _ = step(tr, d, z, plan_for(cuda, "hub", None), mode, layout)
                check_truth(bad, (d, layout, "default pieces"), loss1, dz1, refs)
            clean = step(tr, d, padded(host_matrix(d), cuda), plan, mode)
            for poison in POISONS:
                got = step(tr, d, padded(host_matrix(d), cuda, poison), plan, mode)
                if not (got[0] == clean[0] and all(same(a, b) for a, b in zip(got[1:], clean[1:]))):
                    bad.append((d, "pad columns reach the output", poison))
    assert not bad, bad


@pytest.mark.parametrize("mode", ["sigmoid", "none"])
def test_logits_of_exactly_zero(cuda, mode):
    """zero rows of z and rows with disjoint support (what a ReLU leaves) give logits of exactly 0, where c = w (sigma(0) - y) -- not
    the 1 - y that autograd through max(s, 0) and |s| would give: the fused launch, the default path and the reference agree"""
    d = 12
    x = np.maximum(host_matrix(d), 0).astype(np.float32)
    x[::2, :d // 2] = 0                                                                 # even rows live on the upper columns,
    x[1::2, d // 2:] = 0                                                                # odd rows on the lower ones
    x[:10] = 0                                                                          # and ten rows are dead
    refs = step_references(x, EDGES, LABELS, mode)
    bad = []
    with Trace() as tr:
        for layout in LAYOUTS:
            z = LAYOUTS[layout](x, cuda)
            plan = plan_for(cuda, max_piece=8)
            loss, dz, score, _ = step(tr, layout, z, plan, mode, layout)
            assert int((score == 0).sum()) > 100
            check_truth(bad, (layout, "low-level"), loss, dz, refs)
            for fused in (True, False):
                zg = z.detach().requires_grad_(True)
                tr.expect(layout, z, mode if fused else "given")
                out = edge_bce_loss(zg, plan, activation=mode, fused=fused)
                out.backward()
                check_truth(bad, (layout, "fused" if fused else "unfused"), float(out.detach()), zg.grad, refs)
                if fused and not same(zg.grad, dz):
                    bad.append((layout, "fused path differs from the low-level call"))
    assert not bad, bad


@pytest.mark.parametrize("mode", ["sigmoid", "none"])
def test_saturated_scores_stay_finite(cuda, mode):
    d = 100
    x = host_matrix(d) * np.float32(8.0)                                                # <z_i, z_i> ~ 64 d / 3: far beyond 100
    with Trace() as tr:
        for layout in LAYOUTS:
            z = LAYOUTS[layout](x, cuda)
            loss, dz, score, coef = step(tr, d, z, plan_for(cuda, max_piece=8), mode, layout)
            assert float(score.abs().max()) > 100 and float(score.min()) < -100
            assert np.isfinite(loss) and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(coef).all())
            refs = step_references(x, EDGES, LABELS, mode)
            rep = oracle.truth_report(loss, refs["ref32"][0], refs["truth"][0], cond=refs["cond"][0])
            print(mode, layout, "loss", rep)
            assert rep["ok"], rep


# ---- edge_scores on a plan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [7, 100, 147])
def test_edge_scores_on_a_plan(cuda, d):
    g = np.ascontiguousarray(hash_matrix(1, N_EDGES, seed=9 * d + 1)[0])
    refs = gradient_references(d, False, g)
    gd = torch.from_numpy(g).to(cuda)
    plan = plan_for(cuda, max_piece=8)
    edges = torch.from_numpy(EDGES).to(cuda)
    runs = []
    with Trace() as tr:
        for _ in range(2):
            z = padded(host_matrix(d), cuda).requires_grad_(True)
            tr.expect(d, z, "given")
            out = edge_scores(z, plan)
            assert out.requires_grad
            out.backward(gd)
            runs.append(z.grad)
    assert same(out.detach(), edge_scores(z.detach(), edges)) and same(out.detach(), edge_scores(z.detach(), plan))
    assert same(torch.sigmoid(out.detach()), edge_scores(z.detach(), plan, sigmoid=True))
    assert runs[0].shape == (N_ROWS, d) and same(runs[0], runs[1]), "two backward runs differ"
    rep = oracle.truth_report(runs[0].cpu().numpy(), refs["ref32"][0], refs["truth"][0], cond=refs["cond"][0])
    print(d, rep)
    assert rep["ok"], rep
    with pytest.raises(ValueError):
        edge_scores(z, plan, z2=z.detach().clone())


# ---- the reference fixture ------------------------------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    def __init__(self, z):
        super().__init__()
        self.z = torch.nn.Parameter(z)

    def model_forward(self, idx, device):
        return self.z


class SGCLike(torch.nn.Module):
    """one Linear layer on pre-propagated features, with the reference's model interface"""

    def __init__(self, f_in, hidden):
        super().__init__()
        self._base_model = torch.nn.Linear(f_in, hidden)
        self.x = None

    def preprocess(self, adj, x):
        self.x = x

    def model_forward(self, idx, device):
        return self._base_model(self.x[idx])


def test_train_and_eval_on_the_reference_fixture(cuda, goldens):
    g = goldens.npz("g18_gae_link_prediction")
    pos, neg = g["pos_edges"], g["neg_edges"]
    both = np.concatenate((pos, neg))
    labels = np.concatenate((np.ones(len(pos), np.float32), np.zeros(len(neg), np.float32)))
    n = g["z"].shape[0]
    cond = step_references(g["z"], both, labels, "sigmoid")["cond"]
    model = Stub(padded(g["z"], cuda))
    plan = EdgePlan.from_pos_neg(pos, neg, n, device=cuda)
    loss, roc_auc, avg_prec = edge_predict_train(model, None, plan, torch.optim.SGD(model.parameters(), lr=0.0))
    reps = (oracle.truth_report(loss, g["train|loss"], g["train|loss64"], cond=cond[0]),
            oracle.truth_report(model.z.grad.cpu().numpy(), g["train|grad"], g["train|grad64"], cond=cond[1]))
    print("loss", reps[0], "\ngrad", reps[1], "\nmetrics", (roc_auc, avg_prec), tuple(g["train|metrics"]))
    assert reps[0]["ok"] and reps[1]["ok"], reps
    # the thresholded predictions are the reference's unless a logit is within float32 rounding of 0: d products and d additions, each
    # within 2^-24 of the sum of the absolute terms -- no logit of the fixture is that small
    z64 = g["z"].astype(np.float64)
    s64, c64 = (z64[both[:, 0]] * z64[both[:, 1]]).sum(1), (np.abs(z64[both[:, 0]]) * np.abs(z64[both[:, 1]])).sum(1)
    assert (np.abs(s64) > 2 * z64.shape[1] * 2.0 ** -24 * c64).all()
    tol = len(both) * 2.0 ** -52
    assert abs(roc_auc - g["train|metrics"][0]) <= tol and abs(avg_prec - g["train|metrics"][1]) <= tol
    # edge_predict_eval: ranked as edge_predict_score ranks them; the same scores ranked on the CPU are another float64 summation
    # order of the same rational numbers.  Against the RECORDED values: both metrics depend on the scores only through the order
    # (and ties) between a positive and a negative pair.  That order is the float64 one in the reference's float32 run and in ours
    # whenever the pair's float64 probabilities differ by more than both logits' float32 error -- 2 d roundings of the sum of the
    # absolute terms each, times sigmoid's slope <= 1 / 4 -- plus the rounding of the two float32 sigmoids (8 x 2^-24).  With k
    # pairs closer than that, ROC-AUC moves by at most k / (P N) (one inversion each) and average precision by at most k / P (one
    # positive moves one rank: its precision TP / rank changes by less than 1, weighted 1 / P).
    got = edge_predict_eval(model, None, pos[:100], neg[:100], pos[100:], neg[100:], device=cuda)
    z = model.z.detach()
    d = z64.shape[1]

    def logits64(e):
        a, b = z64[e[:, 0]], z64[e[:, 1]]
        return (a * b).sum(1), 2 * d * 2.0 ** -24 * (np.abs(a) * np.abs(b)).sum(1)

    for k, (p, q) in enumerate(((pos[:100], neg[:100]), (pos[100:], neg[100:]))):
        (sp, ep), (sn, en) = logits64(p), logits64(q)
        gap = np.abs(1 / (1 + np.exp(-sp))[:, None] - 1 / (1 + np.exp(-sn))[None, :]) - 0.25 * (ep[:, None] + en[None, :])
        close = int((gap <= 8 * 2.0 ** -24).sum())
        rounding = (len(p) + len(q)) * 2.0 ** -52
        print("eval set", k, "pairs the float32 order does not pin:", close)
        assert abs(got[2 * k] - g["eval|metrics"][2 * k]) <= close / (len(p) * len(q)) + rounding, (got, g["eval|metrics"])
        assert abs(got[2 * k + 1] - g["eval|metrics"][2 * k + 1]) <= close / len(p) + rounding, (got, g["eval|metrics"])
        scores = edge_scores(z, np.concatenate((p, q)), sigmoid=True)
        y = torch.cat((torch.ones(len(p)), torch.zeros(len(q))))
        assert got[2 * k:2 * k + 2] == binary_ranking_metrics(scores, y.to(cuda))
        on_cpu = binary_ranking_metrics(scores.cpu(), y)
        assert max(abs(a - b) for a, b in zip(got[2 * k:2 * k + 2], on_cpu)) <= 200 * 2.0 ** -52
    print("eval", got, tuple(g["eval|metrics"]))


def test_three_epochs_of_the_task_on_the_reference_fixture(cuda, goldens):
    g = goldens.npz("g18_gae_link_prediction")
    x = torch.from_numpy(g["task|x"]).to(cuda)
    model = SGCLike(x.shape[1], g["task|state|_base_model.bias"].shape[0])
    model.load_state_dict({k[len("task|state|"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("task|state|")})
    split = EdgeSplit(None, *(torch.from_numpy(g[f"task|{s}_edges{t}"]).to(cuda) for s in ("train", "val", "test") for t in ("", "_neg")))
    res = gae_link_prediction(model, split, x, epochs=int(g["task|epochs"]), lr=float(g["task|lr"]), weight_decay=0.0)
    losses = np.array([h["loss"] for h in res.history[:-1]])
    assert len(losses) == 3 and res.history[-1]["epoch"] == "post" and res.split is split
    rep = oracle.truth_report(losses, g["task|loss"], g["task|loss64"], cond=g["task|loss64"])
    print("loss", losses, rep)
    assert rep["ok"], rep
    model.eval()
    with torch.no_grad():
        z = model.model_forward(torch.arange(x.shape[0], device=cuda), cuda)
        scored = torch.cat((split.test_edges, split.train_edges_false, split.val_edges_false, split.test_edges_false))
        logits = edge_scores(z, scored)
    f64 = z.cpu().double()
    e = scored.cpu()
    cond = (f64[e[:, 0]].abs() * f64[e[:, 1]].abs()).sum(1).numpy()
    rep = oracle.truth_report(logits.cpu().numpy(), g["task|logits"], g["task|logits64"], cond=cond)
    print("logits", rep, "pair", (res.test_roc_auc, res.test_avg_prec), tuple(g["task|pair"]))
    assert rep["ok"], rep
    tol = len(scored) * 2.0 ** -52
    assert abs(res.test_roc_auc - g["task|pair"][0]) <= tol and abs(res.test_avg_prec - g["task|pair"][1]) <= tol


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------------
def test_edge_cases_and_wrapper_checks(cuda):
    z = padded(host_matrix(12), cuda)
    empty = EdgePlan(np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.float32), N_ROWS, device=cuda)
    with Trace() as tr:                                               # nothing is launched for E = 0 or d = 0
        dz = dev.edge_loss_grad(z, empty, "sigmoid", dz=torch.full_like(z, float("nan")))
        assert bool((dz == 0).all())
        zg = z.detach().requires_grad_(True)
        loss = edge_bce_loss(zg, empty)
        loss.backward()
        assert float(loss.detach()) == 0.0 and bool((zg.grad == 0).all())
        z0 = z[:, :0].detach().requires_grad_(True)
        plan = plan_for(cuda, max_piece=8)
        for mode in ("sigmoid", "none"):
            loss, scores = edge_bce_loss(z0, plan, activation=mode, return_scores=True)
            loss.backward()
            assert bool((scores == 0).all()) and z0.grad.shape == (N_ROWS, 0)
            want = float(step_references(np.zeros((N_ROWS, 1), np.float32), EDGES, LABELS, mode)["truth"][0])
            assert abs(float(loss) - want) <= 4 * 2.0 ** -24 * want
    plan = plan_for(cuda, max_piece=8)
    with pytest.raises(TypeError):
        edge_bce_loss(z.to(torch.bfloat16), plan)
    with pytest.raises(TypeError):
        dev.edge_loss_grad(z.to(torch.bfloat16), plan, "sigmoid")
    with pytest.raises(ValueError):
        EdgePlan(EDGES, LABELS[:-1], N_ROWS, device=cuda)
    with pytest.raises(ValueError):
        edge_bce_loss(z[:-1], plan)
    with pytest.raises(ValueError):
        dev.edge_loss_grad(z[:-1], plan, "sigmoid")
    with pytest.raises(ValueError):
        edge_bce_loss(z, plan, activation="tanh")
    with pytest.raises(ValueError):
        dev.edge_loss_grad(z, plan, "given")
    with pytest.raises(IndexError):
        EdgePlan(torch.tensor([[0, N_ROWS]], device=cuda), [1.0], N_ROWS, device=cuda)
    # reduction="sum": against the reference's own reduction="sum"
    zg = z.detach().requires_grad_(True)
    total = edge_bce_loss(zg, plan, reduction="sum")
    total.backward()
    bad = []
    check_truth(bad, "sum", float(total), zg.grad, references(12, "sigmoid", reduction="sum"))
    assert not bad, bad
    # one plan serves one step at a time
    a = edge_bce_loss(zg, plan, fused=True)
    edge_bce_loss(zg, plan, fused=True)
    with pytest.raises(RuntimeError):
        a.backward()

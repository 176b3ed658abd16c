"""The edge-score kernel (csrc/sgl_edge.hip), its wrappers and the link-prediction task on a real MI355X: run with `-m gpu`.

Values are compared with the reference's own two expressions, torch.mm(Z, Z.t())[e0, e1], evaluated on the CPU in float32 and in
float64 (the truth) through oracle.truth_report -- at most twice as far from the truth as the reference's float32 result, with the
condition-aware floor for cancelling sums; no tolerance is chosen in this file.  Bit-for-bit claims use torch.equal.  Every launch
runs under torch.profiler: the kernel names seen must be the instances the restated selection rule (edge_scores_common) announces,
and all of them together exactly the compiled ones."""
import numpy as np
import pytest
import torch

import oracle
from edge_scores_common import (DUP, EDGES, N_EDGES, N_ROWS, NEG, REV, SELF, WIDTHS, compiled_instances, expected_instance,
                                gradient_references, host_matrix, parse_edge_kernel_name, references)
from inputs import hash_matrix
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.tricks import binary_ranking_metrics, edge_predict_score, edge_scores, nafs_ensemble_sweep, nafs_link_prediction

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
POISONS = (float("nan"), 1e30)
BIT_WIDTHS = (7, 100, 147, 600)


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


class Trace:
    """Runs launches under torch.profiler and checks, at exit, that the edge_dot_kernel instances that really ran are, in order, the
    ones `expect()` announced; every other kernel is ignored.  A profiler that reports no kernel names fails the comparison."""

    def __init__(self):
        self.expected, self.seen = [], set()

    def expect(self, label, a, b, times=1):
        self.expected += [(label, expected_instance(a, b))] * times

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
        got = [p for p in (parse_edge_kernel_name(e.name) for e in evs) if p is not None]
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


def scores(tr, label, a, b, edges, **kw):
    tr.expect(label, a, a if b is None else b)
    return edge_scores(a, edges, z2=b, **kw)


def same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


def check_truth(bad, label, got, d, two):
    ref32, truth, cond = references(d, two)
    got = got.cpu().numpy()
    if not np.isfinite(got).all():
        bad.append((label, "not finite"))
        return
    rep = oracle.truth_report(got, ref32, truth, cond=cond)
    if not rep["ok"]:
        bad.append((label, rep))


# ---- values, in every compiled instance -------------------------------------------------------------------------------------------------
def test_values_in_every_instance(cuda):
    edges = torch.from_numpy(EDGES).to(cuda)
    bad = []
    with Trace() as tr:
        for d in WIDTHS:
            za, zb = host_matrix(d), host_matrix(d, 1)
            a, b = padded(za, cuda), padded(zb, cuda)
            assert expected_instance(a, a)[1] == 4
            check_truth(bad, ("padded", d), scores(tr, ("padded", d), a, None, edges), d, False)
            check_truth(bad, ("two matrices", d), scores(tr, ("two", d), a, b, edges), d, True)
            av = odd_view(za, cuda)
            assert expected_instance(av, av)[1] == 1
            check_truth(bad, ("odd column view", d), scores(tr, ("view", d), av, None, edges), d, False)
            check_truth(bad, ("padded x odd view", d), scores(tr, ("mixed", d), a, odd_view(zb, cuda), edges), d, True)
            # host edge lists, a pair (u, v), and the low-level call into a caller's output
            got = scores(tr, ("host", d), a, None, EDGES)
            out = torch.full((N_EDGES,), SENTINEL, dtype=torch.float32, device=cuda)
            tr.expect(("edge_dot", d), a, a)
            assert dev.edge_dot(a, a, (EDGES[:, 0], EDGES[:, 1]), out=out) is out
            if not (same(got, out) and same(got, scores(tr, ("device", d), a, None, edges))):
                bad.append((d, "host edges / pair / out="))
    print(f"\n[edge_dot] {len(WIDTHS)} widths, instances seen: {sorted(tr.seen)}")
    assert not bad, (len(bad), bad[:10])
    assert tr.seen == compiled_instances(), sorted(compiled_instances() - tr.seen)


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", [False, True], ids=["padded", "odd-view"])
def test_bits_do_not_depend_on_the_list(cuda, view, monkeypatch):
    edges = torch.from_numpy(EDGES).to(cuda)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(N_EDGES)).to(cuda)
    inv = torch.argsort(perm)
    bad = []
    with Trace() as tr:
        for d in BIT_WIDTHS:
            z = (odd_view if view else padded)(host_matrix(d), cuda)
            base = scores(tr, d, z, None, edges)

            def check(what, got):
                if not same(got, base):
                    bad.append((d, what))

            check("repeated call", scores(tr, d, z, None, edges))
            check("reversed edges", scores(tr, d, z, None, edges[:, [1, 0]].contiguous()))
            check("permuted list", scores(tr, d, z, None, edges[perm])[inv])
            check("two calls", torch.cat((scores(tr, d, z, None, edges[:337]), scores(tr, d, z, None, edges[337:]))))
            check("z2 = z", scores(tr, d, z, z, edges))
            shifted = torch.empty(2 * N_EDGES + 1, dtype=torch.int64, device=cuda)[1:].view(N_EDGES, 2)
            shifted.copy_(edges)
            assert shifted.data_ptr() % 16 == 8 and shifted.is_contiguous()
            check("edge list on an odd 8-byte boundary", scores(tr, d, z, None, shifted))
            for k in (0, 2, 499, 650, 850, 999):
                if not same(scores(tr, d, z, None, edges[k:k + 1]), base[k:k + 1]):
                    bad.append((d, "E = 1", k))
            monkeypatch.setattr(dev, "EDGE_DOT_MAX_EDGES", 300)           # the wrapper's split: 300 + 300 + 300 + 100
            tr.expect(d, z, z, times=4)
            check("split by the wrapper", edge_scores(z, edges))
            monkeypatch.undo()
            if not (same(base[DUP[0]], base[DUP[1]]) and same(base[REV[0]], base[REV[1]]) and same(base[NEG[0]], base[NEG[1]])):
                bad.append((d, "duplicates / reversed twins / negative twins inside one list"))
            # sigmoid=True is torch.sigmoid of the same logits, in place
            if not same(scores(tr, d, z, None, edges, sigmoid=True), torch.sigmoid(base)):
                bad.append((d, "sigmoid"))
    assert not bad, bad


# ---- hostile pads -------------------------------------------------------------------------------------------------------------------------
def test_pad_columns_and_stale_outputs_do_not_reach_the_result(cuda):
    edges = torch.from_numpy(EDGES).to(cuda)
    bad = []
    with Trace() as tr:
        for d in WIDTHS:
            za, zb = host_matrix(d), host_matrix(d, 1)
            a0, b0 = padded(za, cuda), padded(zb, cuda)
            tr.expect(d, a0, b0)
            base = dev.edge_dot(a0, b0, edges)
            for poison in POISONS:
                a, b = padded(za, cuda, poison), padded(zb, cuda, poison)
                out = torch.full((N_EDGES,), SENTINEL, dtype=torch.float32, device=cuda)
                tr.expect(d, a, b)
                dev.edge_dot(a, b, edges, out=out)
                if not same(out, base):
                    bad.append((d, poison))
    assert not bad, bad


# ---- an index outside the matrix: NaN for that edge, never a fault -------------------------------------------------------------------------
@pytest.mark.parametrize("d", [7, 100, 600])
def test_out_of_range_device_index_gives_nan_for_that_edge_only(cuda, d):
    """the kernel's contract for DEVICE index tensors (host lists are refused before the launch): the call returns normally"""
    n = N_ROWS
    e = EDGES.copy()
    where = {3: (n, 0), 64: (0, n), 333: (-n - 1, 5), 500: (5, -n - 1), 998: (2 ** 40, 1), 999: (1, -2 ** 62)}
    for k, pair in where.items():
        e[k] = pair
    good = np.ones(N_EDGES, dtype=bool)
    good[list(where)] = False
    with Trace() as tr:
        for make in (padded, odd_view):
            z = make(host_matrix(d), cuda)
            base = scores(tr, d, z, None, torch.from_numpy(EDGES).to(cuda))
            got = scores(tr, d, z, None, torch.from_numpy(e).to(cuda))
            torch.cuda.synchronize()
            g = torch.from_numpy(good).to(cuda)
            assert bool(torch.isnan(got[~g]).all())
            assert same(got[g], base[g])
    with pytest.raises(IndexError):
        edge_scores(z, e)                                             # the same list from the host: validated there
    # a matrix without rows: every pair is out of range
    empty = torch.empty((0, d), dtype=torch.float32, device=cuda)
    assert bool(torch.isnan(dev.edge_dot(empty, z, torch.zeros((5, 2), dtype=torch.int64, device=cuda))).all())
    assert same(dev.edge_dot(z[:, :0], z[:, :0], torch.from_numpy(e).to(cuda)), torch.zeros(N_EDGES, device=cuda))    # d = 0: zeros


def test_wrapper_checks(cuda):
    z = padded(host_matrix(12), cuda)
    with pytest.raises(TypeError):
        dev.edge_dot(z.to(torch.bfloat16), z.to(torch.bfloat16), EDGES)
    with pytest.raises(TypeError):
        dev.edge_dot(z.cpu(), z, EDGES)
    with pytest.raises(ValueError):
        dev.edge_dot(z, padded(host_matrix(16), cuda), EDGES)
    with pytest.raises(ValueError):
        dev.edge_dot(z, z, EDGES[:, :1])
    with pytest.raises(ValueError):
        dev.edge_dot(z, z, EDGES, out=torch.empty(N_EDGES + 1, device=cuda))
    assert edge_scores(z, np.zeros((0, 2), dtype=np.int64)).shape == (0,)
    assert edge_scores(z, ([], [])).shape == (0,)


# ---- gradients ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True], ids=["same-matrix", "two-matrices"])
@pytest.mark.parametrize("d", [7, 100, 147])
def test_gradients(cuda, d, two):
    g = np.ascontiguousarray(hash_matrix(1, N_EDGES, seed=9 * d + 1)[0])
    refs = gradient_references(d, two, g)
    edges = torch.from_numpy(EDGES).to(cuda)
    gd = torch.from_numpy(g).to(cuda)
    runs = []
    with Trace() as tr:
        for _ in range(2):
            a = padded(host_matrix(d), cuda).requires_grad_(True)
            b = padded(host_matrix(d, 1), cuda).requires_grad_(True) if two else None
            out = scores(tr, d, a, b, edges)
            assert out.requires_grad
            out.backward(gd)
            runs.append((a.grad, None if b is None else b.grad))
    for k in range(2 if two else 1):
        got = runs[0][k]
        assert got.shape == (N_ROWS, d) and bool(torch.isfinite(got).all())
        assert same(runs[0][k], runs[1][k]), "two backward runs differ"
        rep = oracle.truth_report(got.cpu().numpy(), refs["ref32"][k], refs["truth"][k], cond=refs["cond"][k])
        print(d, two, "dA" if k == 0 else "dB", rep)
        assert rep["ok"], rep
    # the forward of the gradient-carrying path is the plain one, bit for bit
    with Trace() as tr, torch.no_grad():
        assert same(out.detach(), scores(tr, d, a.detach(), None if b is None else b.detach(), edges))


# ---- the task ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["mean", "max", "concat", "simple"])
def test_nafs_link_prediction_on_the_reference_fixture(cuda, goldens, method):
    g = goldens.npz("g14_link_prediction")
    adj = goldens.graph("pl256")
    x, hops, r_list = g["x"], [int(h) for h in g["hops"]], [float(r) for r in g["r_list"]]
    pos, neg = g["pos_edges"], g["neg_edges"]
    both = np.concatenate((pos, neg))
    labels = torch.cat((torch.ones(len(pos)), torch.zeros(len(neg))))
    feats = nafs_ensemble_sweep(adj, x, hops, r_list=r_list, method=method)
    with Trace() as tr:
        for h in hops:                                                # the task's own launches: same shapes, same allocator
            tr.expect(("task", h), feats[h], feats[h])
        res = nafs_link_prediction(adj, x, hops, torch.from_numpy(pos), torch.from_numpy(neg), r_list=r_list, method=method,
                                   return_scores=True)
        mine = {}
        for h in hops:
            tr.expect(("after", h), feats[h], feats[h], times=3)
            mine[h] = (edge_predict_score(feats[h], pos, neg, 0.5), edge_scores(feats[h], both, sigmoid=True), edge_scores(feats[h], both))
    assert sorted(res.metrics) == hops
    bad = []
    for h in hops:
        key = f"lp|{method}|hops{h}"
        assert res.metrics[h] == binary_ranking_metrics(res.scores[h], labels.to(cuda))
        # the same scores ranked on the CPU: another float64 summation order of the same rational numbers
        on_cpu = binary_ranking_metrics(res.scores[h].cpu(), labels)
        assert max(abs(p - q) for p, q in zip(res.metrics[h], on_cpu)) <= len(both) * 2.0 ** -52, (res.metrics[h], on_cpu)
        assert res.metrics[h] == mine[h][0]
        assert same(res.scores[h], mine[h][1])
        logits = mine[h][2]
        f64 = feats[h].cpu().double()
        cond = (f64[both[:, 0]].abs() * f64[both[:, 1]].abs()).sum(1).numpy()
        reps = (oracle.parity_report(logits.cpu().numpy(), g[key + "|logits"], tol=1e-5, scale=cond),
                oracle.parity_report(res.scores[h].cpu().numpy(), g[key + "|probs"], tol=1e-5, scale=cond))
        print(key, "logits", reps[0]["max_abs_over_max"], reps[0]["row_l2_rel"], "probs", reps[1]["max_abs_over_max"], reps[1]["row_l2_rel"],
              "metrics", res.metrics[h], tuple(g[key + "|metrics"]))
        if not (reps[0]["ok"] and reps[1]["ok"]):
            bad.append((key, reps))
    assert not bad, bad
    # the best-hop bookkeeping of LinkPredictionNAFS._execute: strictly greater wins, the bests start at 0
    best = [0.0, 0.0, 0, 0]
    for h in hops:
        if res.metrics[h][0] > best[0]:
            best[0], best[2] = res.metrics[h][0], h
        if res.metrics[h][1] > best[1]:
            best[1], best[3] = res.metrics[h][1], h
    assert (res.test_roc_auc, res.test_avg_prec, res.best_hop_roc_auc, res.best_hop_avg_prec) == tuple(best)

"""Link prediction from node features, on the MI355X, without the N x N similarity matrix.

Reference: LinkPredictionNAFS (sgl/tasks/link_prediction.py:159-284) ends every hop count with

    sim = torch.mm(input_features, input_features.t())                              # [N, N]            (line 282)
    roc_auc, avg_prec = edge_predict_score(sim, test_edges, test_edges_neg, thr)    # sim[e0, e1] -> sigmoid -> AUC / AP  (283)

(sgl/tasks/utils.py:263-271), and edge_predict_train does the same under autograd (sgl/tasks/utils.py:281-285).  Of the N^2
products E are read.  Here the E scores are computed directly (device.edge_dot: one kernel, two row gathers and a dot product per
edge), the sigmoid is one in-place pass over E floats, and the two ranking metrics -- sklearn's roc_auc_score and
average_precision_score in the reference -- are a sort and two prefix sums in torch, on the device the scores are on.

The backward of the scores needs no kernel of its own and no atomics: dZ[i] = sum over the edges at i of g_e * (the other row) is a
sparse-times-dense product, so the (u, v, g) triplets become a CSR matrix (sgl_coo_to_csr: duplicates summed in input order) and the
library's SpMM does the rest -- deterministic like every product it computes."""
from collections import namedtuple

import numpy as np
import torch

from .. import device as dev
from .nafs_features import nafs_ensemble_sweep

__all__ = ["edge_scores", "binary_ranking_metrics", "edge_predict_score", "nafs_link_prediction", "LinkPredictionResult"]


def _grad_spmm(rows, cols, vals, n_rows, n_cols, x):
    """(the [n_rows, n_cols] matrix of the triplets, duplicates summed in input order) @ x"""
    from ..io import coo_to_csr_device
    g = coo_to_csr_device(rows, cols, vals, n_rows, device=x.device, num_col=n_cols)
    x = x if _kernel_ready(x) else x.contiguous()
    return dev.DeviceCSR(g.rowptr, g.col, g.val, g.shape).spmm(x)


def _kernel_ready(t):
    return t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])


def _wrapped(idx, n):
    return torch.where(idx < 0, idx + n, idx)


class _EdgeDot(torch.autograd.Function):
    """out[e] = <a[u_e], b[v_e]>; `same`: b is a (one gradient, from the symmetrised triplets)"""

    @staticmethod
    def forward(ctx, a, b, edges, same):
        ctx.same = same
        ctx.save_for_backward(a, b, edges)
        return dev.edge_dot(a, a if same else b, edges)

    @staticmethod
    def backward(ctx, g):
        a, b, edges = ctx.saved_tensors
        g = g.contiguous().to(torch.float32)
        u, v = _wrapped(edges[:, 0], a.shape[0]), _wrapped(edges[:, 1], a.shape[0] if ctx.same else b.shape[0])
        da = db = None
        if ctx.same:
            if ctx.needs_input_grad[0]:
                # d<z_u, z_v> = g z_v at row u and g z_u at row v (a self pair: 2 g z_u): dZ = G_sym Z, G_sym from [(u, v, g) ..., (v, u, g) ...]
                n = a.shape[0]
                da = _grad_spmm(torch.cat((u, v)), torch.cat((v, u)), torch.cat((g, g)), n, n, a)
        else:
            if ctx.needs_input_grad[0]:
                da = _grad_spmm(u, v, g, a.shape[0], b.shape[0], b)                 # dA = G B
            if ctx.needs_input_grad[1]:
                db = _grad_spmm(v, u, g, b.shape[0], a.shape[0], a)                 # dB = G^T A
        return da, db, None, None


def edge_scores(z, edges, z2=None, sigmoid=False):
    """The link-prediction logits of an edge list, [E] float32 on the device: <z[u_e], z2[v_e]> (z2 = z when not given) -- the entries
    `torch.mm(z, z2.t())[edges[:, 0], edges[:, 1]]` of the reference (tasks/link_prediction.py:282-283, tasks/utils.py:281-285).
    edges: [E, 2] (tensor or ndarray, host or device) or a pair (u, v) of index sequences; negative indices count from the end.  Host
    indices are validated (IndexError); in a device tensor a pair outside the matrices scores NaN.
    sigmoid=True applies torch.sigmoid_ to the logits in place (what the reference's torch.sigmoid makes of the same logits).
    When z (or z2) requires grad the scores carry it: the backward is one SpMM per gradient with the matrix of the (u, v, g)
    triplets -- no atomics, two runs are bit-equal (a device index outside the matrices raises there)."""
    same = z2 is None or z2 is z
    b = z if same else z2
    if torch.is_grad_enabled() and (z.requires_grad or b.requires_grad):
        dev._no_bf16("edge_scores", z, b)
        dev._check_mat(z, "z")
        dev._check_mat(b, "z2")
        e = dev._device_edges(edges, z.shape[0], b.shape[0], z.device)
        out = _EdgeDot.apply(z, b, e, same)
        return torch.sigmoid(out) if sigmoid else out
    out = dev.edge_dot(z, b, edges)
    return torch.sigmoid_(out) if sigmoid else out


def binary_ranking_metrics(scores, labels):
    """(roc_auc, avg_prec) of binary labels ranked by `scores`: sklearn's roc_auc_score and average_precision_score (what
    edge_predict_score calls, sgl/tasks/utils.py:269-270) in plain torch, in float64, on the device the scores are on (CPU included).
    Tie-aware as sklearn is: the scores are sorted descending and equal scores form one group; with (FP, TP) the counts at the END
    of each group,
        roc_auc  = trapezoid area under the (FP, TP) points from (0, 0), divided by P N
        avg_prec = sum over the groups of (TP - TP_before) / P * TP / (TP + FP).
    One class only raises ValueError, as sklearn's roc_auc_score does."""
    s = torch.as_tensor(scores).detach().reshape(-1).to(torch.float64)
    y = torch.as_tensor(labels).detach().reshape(-1).to(s.device)
    if s.numel() != y.numel():
        raise ValueError("scores and labels must have the same length")
    y = (y != 0).to(torch.int64)
    n = int(s.numel())
    pos = int(y.sum()) if n else 0
    neg = n - pos
    if pos == 0 or neg == 0:
        raise ValueError("Only one class present in labels. ROC AUC score is not defined in that case.")
    s, order = torch.sort(s, descending=True)
    y = y[order]
    ends = torch.ones(n, dtype=torch.bool, device=s.device)            # last element of every group of equal scores
    ends[:-1] = s[:-1] != s[1:]
    tp = torch.cumsum(y, 0)[ends]
    fp = torch.nonzero(ends).reshape(-1) + 1 - tp
    zero = torch.zeros(1, dtype=torch.int64, device=s.device)
    tp0, fp0 = torch.cat((zero, tp[:-1])), torch.cat((zero, fp[:-1]))
    area2 = int(((fp - fp0) * (tp + tp0)).sum())                         # twice the area, exact in integers
    roc_auc = area2 / (2.0 * pos * neg)
    avg_prec = float((((tp - tp0).to(torch.float64) / pos) * (tp.to(torch.float64) / (tp + fp).to(torch.float64))).sum())
    return roc_auc, avg_prec


def _edge_matrix(edges):
    t = edges if torch.is_tensor(edges) else torch.from_numpy(np.asarray(edges))
    if t.numel() == 0:
        t = t.reshape(0, 2)
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError("edges must be [E, 2]")
    return t.to(torch.int64)


def _scored_edges(pos_edges, neg_edges, device):
    """(all edges [P + Q, 2], labels ones then zeros on `device`): torch.cat((pos, neg)) of sgl/tasks/utils.py:264-265"""
    pos, neg = _edge_matrix(pos_edges), _edge_matrix(neg_edges)
    if pos.is_cuda or neg.is_cuda:
        pos, neg = pos.to(device), neg.to(device)
    labels = torch.cat((torch.ones(len(pos), device=device), torch.zeros(len(neg), device=device)))
    return torch.cat((pos, neg)), labels


def edge_predict_score(z, pos_edges, neg_edges, threshold=None):
    """edge_predict_score of the reference (sgl/tasks/utils.py:263-271) with the node features z in place of its N x N
    `edge_feature = z z^T`: sigmoid scores of the positive then the negative edges, labels ones then zeros, (roc_auc, avg_prec).
    `threshold` is accepted and unused, as in the reference (its thresholding line is commented out)."""
    edges, labels = _scored_edges(pos_edges, neg_edges, z.device)
    with torch.no_grad():
        return binary_ranking_metrics(edge_scores(z, edges, sigmoid=True), labels)


LinkPredictionResult = namedtuple("LinkPredictionResult", ["metrics", "best_hop_roc_auc", "best_hop_avg_prec", "test_roc_auc",
                                                           "test_avg_prec", "scores"])
LinkPredictionResult.__doc__ = """nafs_link_prediction's result: metrics = {hop count: (roc_auc, avg_prec)}; the four values
LinkPredictionNAFS keeps (best_hop_roc_auc, best_hop_avg_prec, test_roc_auc, test_avg_prec); scores = {hop count: sigmoid scores
[P + Q] on the device} when asked for, else None"""


@torch.no_grad()
def nafs_link_prediction(train_adj, x, hops, test_edges, test_edges_neg, r_list=(0.5, 0.4, 0.3, 0.2, 0.1, 0), method="mean",
                         threshold=0.5, device="cuda", strict_order=False, reorder=None, return_scores=False):
    """LinkPredictionNAFS._execute (sgl/tasks/link_prediction.py:203-284) for a given edge split: for every hop count of `hops` (an
    int = range(hops), or a list) the NAFS ensemble features of the training graph, the sigmoid scores of the test edges followed by
    the negative ones, and their (roc_auc, avg_prec); then the best-hop bookkeeping of lines 207-231 (strictly greater wins, so
    the smallest best hop count; the bests start at 0).  One nafs_ensemble_sweep -- one propagation per r for ALL hop counts -- whose
    consumer scores each feature matrix as soon as its ensemble is complete; only E floats per hop count outlive it.
    The edge split (mask_test_edges, line 176) stays the caller's job.  Returns a LinkPredictionResult."""
    device = torch.device(device)
    edges, labels = _scored_edges(test_edges, test_edges_neg, device)
    n = int(x.shape[0])
    edges = dev._device_edges(edges, n, n, device)                                   # validated (host indices) and uploaded once
    kept = {} if return_scores else None

    def score(hop, feats):
        s = edge_scores(feats, edges, sigmoid=True)
        if kept is not None:
            kept[hop] = s
        return binary_ranking_metrics(s, labels)

    metrics = nafs_ensemble_sweep(train_adj, x, hops, r_list=r_list, method=method, device=device, strict_order=strict_order,
                                  reorder=reorder, consume=score)
    best_roc_auc, best_avg_prec = 0., 0.
    best_hop_roc_auc, best_hop_avg_prec = 0, 0
    for hop in (range(hops) if isinstance(hops, int) else hops):
        roc_auc, avg_prec = metrics[int(hop)]
        if roc_auc > best_roc_auc:
            best_roc_auc, best_hop_roc_auc = roc_auc, hop
        if avg_prec > best_avg_prec:
            best_avg_prec, best_hop_avg_prec = avg_prec, hop
    return LinkPredictionResult(metrics, best_hop_roc_auc, best_hop_avg_prec, best_roc_auc, best_avg_prec, kept)

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

__all__ = ["edge_scores", "binary_ranking_metrics", "edge_predict_score", "nafs_link_prediction", "LinkPredictionResult",
           "has_edges", "mask_test_edges", "EdgeSplit"]


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
    The edge split (line 176) is mask_test_edges below: its adj_train, test_edges and test_edges_false are this function's first,
    fourth and fifth argument, on the device as they are.  Returns a LinkPredictionResult."""
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


# ---- the edge split: mask_test_edges of the reference (sgl/tasks/utils.py:148-259) on the device --------------------------------------
EdgeSplit = namedtuple("EdgeSplit", ["adj_train", "train_edges", "train_edges_false", "val_edges", "val_edges_false", "test_edges",
                                     "test_edges_false"])
EdgeSplit.__doc__ = """mask_test_edges' result, in the order of the reference's 7-tuple: adj_train (a DeviceAdjacency) and six int64
[*, 2] edge lists on the device"""

_SHUFFLE_STREAM, _GOLD = 101, 0x9E3779B97F4A7C15       # the hash of csrc/sgl_hash.h (numpy mirror: synthetic._hash4)
_NEGATIVE_SETS = ("train", "test", "val")               # the order in which the reference fills them
MAX_ROUND_CANDIDATES = 1 << 25                          # candidates of one round: 24 bytes each, plus the sort of their keys


def _u64(x):
    """a Python integer as the int64 with the same 64 bits"""
    x &= 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >> 63 else x


def _lsr(z, k):
    """logical right shift of the 64 bits held in an int64 tensor"""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix64(z):
    if not torch.is_tensor(z):                                                       # a Python integer: exact, then wrapped
        z = (z + _GOLD) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)
    z = z + _u64(_GOLD)                                                              # int64 tensors wrap: the same 64 bits
    z = (z ^ _lsr(z, 30)) * _u64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _u64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def _hash4(seed, stream, a, b):
    """h(seed, stream, a, b) of csrc/sgl_hash.h for an int64 tensor a and an integer b: the 64 bits, held in an int64 tensor"""
    head = _mix64(((int(seed) & 0xFFFFFFFFFFFFFFFF) * _GOLD + stream) & 0xFFFFFFFFFFFFFFFF)
    return _mix64(_mix64(a ^ _u64(head)) + b)


def _shuffle_order(seed, n_edges, device):
    """stable argsort of h(seed, 101, e, 0) read as unsigned, e = 0 .. n_edges - 1"""
    h = _hash4(seed, _SHUFFLE_STREAM, torch.arange(n_edges, dtype=torch.int64, device=device), 0)
    return torch.sort(h ^ _u64(1 << 63), stable=True)[1]                             # flipping the top bit: unsigned order as signed


def _device_adjacency(adj, device):
    from ..io import DeviceAdjacency
    if isinstance(adj, DeviceAdjacency):
        return adj
    return DeviceAdjacency.from_scipy(adj, device=device)


@torch.no_grad()
def has_edges(adj, edges, device="cuda"):
    """bool [Q] on the device: is edges[q] = (u, v) a stored entry of adj?  adj: a scipy matrix (uploaded to `device`) or a
    DeviceAdjacency (used where it is); edges as for edge_scores.  One search inside a CSR row per pair (device.csr_find) -- the
    membership test of the reference's `edges_all_set` (sgl/tasks/utils.py:166-168) without the set.  An explicitly stored zero
    counts as stored."""
    return dev.csr_find(_device_adjacency(adj, device), edges) >= 0


def _positive_entries(adj):
    """(DeviceAdjacency of the stored off-diagonal non-zero entries of adj, their rows int64 [nnz]): what `adj - diag(adj)` followed
    by eliminate_zeros() leaves (sgl/tasks/utils.py:154-155); adj itself when there is nothing to drop"""
    from ..io import DeviceAdjacency
    n = adj.shape[0]
    dv = adj.rowptr.device
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dv), adj.rowptr[1:] - adj.rowptr[:-1])
    keep = (rows != adj.col) & (adj.val != 0)
    if bool(keep.all()):
        return adj, rows
    rows = rows[keep]
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dv)
    torch.cumsum(torch.bincount(rows, minlength=n), 0, out=rowptr[1:])
    return DeviceAdjacency(rowptr, adj.col[keep], adj.val[keep], adj.shape), rows


def _draw_negatives(pos, seed, need, round_size, max_draws):
    """the first `need` accepted candidates of the stream over the positive matrix `pos`, in stream order: int64 [need, 2].
    Candidate t is accepted iff its key is >= 0 and no accepted candidate before it has that key -- so acceptance depends on the
    candidates before t alone, and rounds of any size give the same list."""
    dv = pos.rowptr.device
    taken = torch.empty(0, dtype=torch.int64, device=dv)                             # keys accepted so far, sorted
    found, have, drawn = [], 0, 0
    while have < need:
        if drawn >= max_draws:
            raise RuntimeError(f"mask_test_edges: {have} of {need} negative edges after {drawn} candidates (max_draws): the graph has "
                               "too few pairs that are not edges, or max_draws is too small")
        left = need - have
        count = int(round_size) if round_size else min(max(left + left // 4, 4096), MAX_ROUND_CANDIDATES)
        count = min(max(count, 1), max_draws - drawn)
        edges, key = dev.edge_candidates(pos, seed, drawn, count)
        drawn += count
        at = torch.nonzero(key >= 0).reshape(-1)                                     # positions of the valid candidates, ascending
        k, by_key = torch.sort(key[at], stable=True)                                 # equal keys keep their stream order
        first = torch.ones(k.numel(), dtype=torch.bool, device=dv)
        first[1:] = k[1:] != k[:-1]                                                  # the earliest candidate of every key
        k, by_key = k[first], by_key[first]
        if taken.numel():
            slot = torch.searchsorted(taken, k).clamp_(max=taken.numel() - 1)
            fresh = taken[slot] != k
            k, by_key = k[fresh], by_key[fresh]
        at = torch.sort(at[by_key])[0][:left]                                        # back in stream order; no more than are missing
        if at.numel():
            found.append(edges[at])
            have += int(at.numel())
            taken = torch.sort(torch.cat((taken, key[at])))[0]
    return torch.cat(found) if found else torch.empty((0, 2), dtype=torch.int64, device=dv)


@torch.no_grad()
def mask_test_edges(adj, seed=0, device="cuda", negatives=_NEGATIVE_SETS, round_size=None, max_draws=None):
    """mask_test_edges of the reference (sgl/tasks/utils.py:148-259) on the device, seeded: 10 % of the undirected edges for testing,
    5 % for validation, the rest for training, an equal number of negative pairs for each, and the training adjacency.  adj: a square
    scipy matrix (uploaded to `device`) or a DeviceAdjacency.  Returns an EdgeSplit, which unpacks like the reference's 7-tuple;
    adj_train is a DeviceAdjacency, the six edge lists are int64 [*, 2] device tensors -- what nafs_link_prediction takes.

    Positive entries are the stored off-diagonal ones with a non-zero value (the reference subtracts the diagonal and calls
    eliminate_zeros(); nothing dense is built here and nothing asserted).  `edges` are those with row < col in CSR order (sp.triu),
    E of them; num_test = E // 10, num_val = E // 20.  The shuffle is order = stable argsort of h(seed, 101, e, 0) (csrc/sgl_hash.h);
    val = edges[order[:num_val]], test = edges[order[num_val:num_val + num_test]], train = the other edges in their order (np.delete).
    adj_train = T + T^T with every value 1.0, T the matrix of the train edges.

    Negatives come from ONE stream of candidate pairs (device.edge_candidates, stream 102 of the same hash), filled in the reference's
    order -- train, then test, then val, each as long as its positive list; a set not named in `negatives` is skipped and comes back
    [0, 2].  A candidate (i, j) is accepted iff i != j, (i, j) is not a positive entry (in the drawn orientation, as in the reference)
    and neither orientation of it has been accepted before, in this set or an earlier one; the pairs are returned as drawn, in stream
    order.  The reference's val set may repeat itself (its `in np.array(a set)` test is always False); this one never does.
    round_size: candidates per round (default: a quarter more than are missing); the result does not depend on it.

    Where the reference would loop for ever: ValueError when more negatives are asked for than there are unordered pairs with an
    orientation that is not an edge; RuntimeError when the stream has not filled the sets after max_draws candidates (default
    64 x the number needed + 65536)."""
    device = torch.device(device)
    adj = _device_adjacency(adj, device)
    n = adj.shape[0]
    if adj.shape[1] != n:
        raise ValueError("mask_test_edges: the adjacency matrix must be square")
    unknown = [s for s in negatives if s not in _NEGATIVE_SETS]
    if unknown:
        raise ValueError(f"mask_test_edges: negatives must name sets of {_NEGATIVE_SETS}, not {unknown}")
    dv = adj.rowptr.device
    pos, rows = _positive_entries(adj)
    upper = rows < pos.col
    edges = torch.stack((rows[upper], pos.col[upper].to(torch.int64)), dim=1)        # sp.triu in CSR order
    n_edges = int(edges.shape[0])
    num_test, num_val = n_edges // 10, n_edges // 20
    order = _shuffle_order(seed, n_edges, dv)
    val_edges, test_edges = edges[order[:num_val]], edges[order[num_val:num_val + num_test]]
    in_train = torch.ones(n_edges, dtype=torch.bool, device=dv)
    in_train[order[:num_val + num_test]] = False
    train_edges = edges[in_train]

    from ..io import DeviceAdjacency, coo_to_csr_device
    if train_edges.shape[0]:
        adj_train = coo_to_csr_device(torch.cat((train_edges[:, 0], train_edges[:, 1])), torch.cat((train_edges[:, 1], train_edges[:, 0])),
                                      torch.ones(2 * train_edges.shape[0], dtype=torch.float32, device=dv), n, device=dv)
    else:
        adj_train = DeviceAdjacency(torch.zeros(n + 1, dtype=torch.int64, device=dv), torch.empty(0, dtype=torch.int32, device=dv),
                                    torch.empty(0, dtype=torch.float32, device=dv), (n, n))

    sizes = {"train": int(train_edges.shape[0]), "test": num_test, "val": num_val}
    wanted = [s for s in _NEGATIVE_SETS if s in negatives]
    need = sum(sizes[s] for s in wanted)
    false = {s: torch.empty((0, 2), dtype=torch.int64, device=dv) for s in _NEGATIVE_SETS}
    if need:
        both = int((dev.csr_find(pos, edges.flip(1)) >= 0).sum())                    # pairs stored in both orientations: never drawable
        room = n * (n - 1) // 2 - both
        if need > room:
            raise ValueError(f"mask_test_edges: {need} negative edges asked for, the graph has {room} pairs of nodes with an orientation "
                             "that is not an edge")
        max_draws = 64 * need + 65536 if max_draws is None else int(max_draws)
        drawn = _draw_negatives(pos, seed, need, round_size, max_draws)
        lo = 0
        for s in wanted:
            false[s] = drawn[lo:lo + sizes[s]]
            lo += sizes[s]
    return EdgeSplit(adj_train, train_edges, false["train"], val_edges, false["val"], test_edges, false["test"])

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
           "has_edges", "mask_test_edges", "EdgeSplit",
           "EdgePlan", "edge_bce_loss", "edge_predict_train", "edge_predict_eval", "gae_link_prediction", "GAELinkPredictionResult"]


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
    triplets -- no atomics, two runs are bit-equal (a device index outside the matrices raises there).
    edges may also be an EdgePlan (z2 must then be z): the same forward, and a backward that is ONE launch over the prepared list
    (sgl_edge_loss_grad_f32 with the upstream gradient as the coefficients) -- no sort and no new CSR per step."""
    if isinstance(edges, EdgePlan):
        if not (z2 is None or z2 is z):
            raise ValueError("edge_scores: an EdgePlan scores one matrix against itself (z2 must be z)")
        if torch.is_grad_enabled() and z.requires_grad:
            dev._no_bf16("edge_scores", z)
            dev._check_mat(z, "z")
            edges._check_z(z, "edge_scores")
            out = _EdgeDotPlanned.apply(z, edges)
            return torch.sigmoid(out) if sigmoid else out
        edges._check_z(z, "edge_scores")
        edges = edges.edges
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


# ---- the trainable task: LinkPredictionGAE of the reference (sgl/tasks/link_prediction.py:14-157) ---------------------------------------
class EdgePlan:
    """An edge list with labels, prepared ONCE for every training step on it (the edge list of a training run never changes):

        plan = EdgePlan(edges, labels, n)            # or EdgePlan.from_pos_neg(pos, neg, n): cat(pos, neg), labels 1 .. 1, 0 .. 0
        loss = edge_bce_loss(z, plan)                # every epoch: nothing sorted, no new CSR, no atomics (paths: see edge_bce_loss)

    edges: [E, 2] integers or a pair (u, v), host or device; labels: [E] float32 (soft labels are allowed); n: the number of nodes.
    Negative indices are wrapped HERE and an index outside [-n, n) raises IndexError here, for device tensors too (one min / max
    reduction on the setup path): the kernel has no bad-index path.  max_piece: incidences per piece (None: device.EDGE_LOSS_MAX_PIECE).
    device: where the tables live; "cpu" builds the same tables with the same torch ops (index arithmetic only).

    Tables (device.edge_incidence, device.edge_pieces): inc_ptr int64 [n + 1], inc_other int32 [2 E], inc_edge int64 [2 E] -- the
    incidences grouped by node, ascending by edge position inside a node, a self pair's two entries both there, primary first,
    duplicates separate -- and pieces [P, 4] / fold [F, 3]: rows cut into pieces of at most max_piece incidences; a row that is one
    piece writes dZ[row], the pieces of a cut row write rows of a partial buffer that are added in piece order, without atomics.
    Also kept: edges (wrapped, int64 [E, 2]), labels, and the buffers of a step -- piece_loss, coef, score, and per width the partial
    rows and the fused path's dZ -- allocated once.  They serve ONE step at a time: a backward after another forward on the same
    plan raises.  (The default, unfused path of edge_bce_loss hands autograd a dZ of its own every step: see there.)"""

    def __init__(self, edges, labels, n, max_piece=None, device="cuda"):
        device = _indexed(device)
        n = int(n)
        if n < 0 or n >= 2 ** 31:
            raise ValueError("EdgePlan: n must be in [0, 2^31)")
        e = _plan_edges(edges, device)
        if e.shape[0]:
            lo, hi = int(e.min()), int(e.max())
            if lo < -n or hi >= n:
                raise IndexError("index out of range in edge list")
        e = _wrapped(e, n).contiguous()
        labels = torch.as_tensor(labels)
        if labels.dim() != 1 or labels.numel() != e.shape[0]:
            raise ValueError(f"EdgePlan: labels must be [E] = [{e.shape[0]}], got {tuple(labels.shape)}")
        self.n, self.n_edges = n, int(e.shape[0])
        self.edges = e
        self.labels = labels.to(device=device, dtype=torch.float32).contiguous()
        self.max_piece = dev.EDGE_LOSS_MAX_PIECE if max_piece is None else int(max_piece)
        self.inc_ptr, self.inc_other, self.inc_edge = dev.edge_incidence(e[:, 0], e[:, 1], n)
        self.pieces, self.fold, self.n_partial = dev.edge_pieces(self.inc_ptr, self.max_piece)
        self.n_pieces = int(self.pieces.shape[0])
        self.piece_loss = torch.zeros(self.n_pieces, dtype=torch.float32, device=device)
        self.coef = torch.zeros(self.n_edges, dtype=torch.float32, device=device)
        self.score = torch.zeros(self.n_edges, dtype=torch.float32, device=device)
        self.device = device
        self._partial, self._dz, self.step = {}, {}, 0

    @classmethod
    def from_pos_neg(cls, pos_edges, neg_edges, n, max_piece=None, device="cuda"):
        """the reference's layout (sgl/tasks/utils.py:282-283): torch.cat((pos, neg)) with labels ones then zeros"""
        device = _indexed(device)
        pos, neg = _plan_edges(pos_edges, device), _plan_edges(neg_edges, device)
        labels = torch.cat((torch.ones(len(pos), device=device), torch.zeros(len(neg), device=device)))
        return cls(torch.cat((pos, neg)), labels, n, max_piece=max_piece, device=device)

    def partial_rows(self, d):
        """the [n_partial, d] buffer the pieces of cut rows write (None when no row is cut), allocated once per width"""
        if self.n_partial == 0:
            return None
        if d not in self._partial:
            self._partial[d] = dev.alloc_rows(self.n_partial, d, self.device)
        return self._partial[d]

    def dz_rows(self, d):
        if d not in self._dz:
            self._dz[d] = dev.alloc_rows(self.n, d, self.device)
        return self._dz[d]

    def _check_z(self, z, who):
        if z.dim() != 2 or z.shape[0] != self.n:
            raise ValueError(f"{who}: z must be [{self.n}, d] (the plan's node count), got {tuple(z.shape)}")
        if z.device != self.device:
            raise ValueError(f"{who}: z is on {z.device}, the plan on {self.device}")


def _indexed(device):
    """torch.device(device), "cuda" as the current device with its index (what the tensors on it report)"""
    device = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if device.type == "cuda" and device.index is None else device


def _plan_edges(edges, device):
    """an edge list of any kind as int64 [E, 2] on `device`, indices as given (EdgePlan validates and wraps them itself)"""
    if isinstance(edges, (tuple, list)) and len(edges) == 2 and not (torch.is_tensor(edges) or isinstance(edges, np.ndarray)):
        u, v = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).reshape(-1) for t in edges)
        if u.shape != v.shape:
            raise ValueError("EdgePlan: u and v must be of one length")
        edges = torch.stack((u.to(device=device, dtype=torch.int64), v.to(device=device, dtype=torch.int64)), dim=1)
    t = edges if torch.is_tensor(edges) else torch.from_numpy(np.asarray(edges))
    if t.numel() == 0:
        t = t.reshape(0, 2)
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError("EdgePlan: edges must be [E, 2] (or a pair (u, v))")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("EdgePlan: edges must be integers")
    return t.to(device=device, dtype=torch.int64)


class _EdgeDotPlanned(torch.autograd.Function):
    """edge scores of a prepared list: the forward of _EdgeDot, the backward one GIVEN-mode launch"""

    @staticmethod
    def forward(ctx, z, plan):
        ctx.plan = plan
        ctx.save_for_backward(z)
        return dev.edge_dot(z, z, plan.edges)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        return dev.edge_loss_grad(z, ctx.plan, "given", given=g.contiguous().to(torch.float32)), None


def _bce_terms(s, y, activation):
    """(L, c) per edge in torch, c = dL / ds WITHOUT the weight w: the formulas of csrc/sgl_edge_loss.hip, formed from e = exp(-|s|)
    like there -- not by autograd through max / abs, whose subgradients at s = 0 are not sigma(s) - y"""
    e = torch.exp(-s.abs())
    r = 1.0 / (1.0 + e)
    sig = torch.where(s >= 0, r, e * r)                                              # sigma(s)
    if activation == "sigmoid":
        ep = torch.exp(-sig)
        return (1 - y) * sig + torch.log1p(ep), (1.0 / (1.0 + ep) - y) * (e * r * r)
    return torch.clamp(s, min=0) - s * y + torch.log1p(e), torch.where(s >= 0, (1 - y) - e * r, sig - y)


def _loss_of(scores, plan, activation, w):
    return (_bce_terms(scores, plan.labels, activation)[0].double().sum() * w).to(torch.float32)


class _ZeroGrad(torch.autograd.Function):
    """a constant that hangs on z in the graph: its gradient is exact zeros whatever z holds (E = 0, d = 0)"""

    @staticmethod
    def forward(ctx, z, value):
        ctx.shape = z.shape
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return g.new_zeros(ctx.shape), None


class _EdgeBCEUnfused(torch.autograd.Function):
    """plan reuse without fusing: device.edge_dot into the plan's score buffer, loss and coefficients by _bce_terms on E floats (the
    coefficients into the plan's coef buffer), and in the backward ONE GIVEN-mode launch with g x coef"""

    @staticmethod
    def forward(ctx, z, plan, activation, w):
        plan.step += 1
        ctx.plan, ctx.step = plan, plan.step
        ctx.save_for_backward(z)
        dev.edge_dot(z, z, plan.edges, out=plan.score)
        terms, coef = _bce_terms(plan.score, plan.labels, activation)
        torch.mul(coef, w, out=plan.coef)
        ctx.mark_non_differentiable(plan.score)
        return (terms.double().sum() * w).to(torch.float32), plan.score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gs):
        if ctx.plan.step != ctx.step:
            raise RuntimeError("edge_bce_loss: the plan ran another step since this forward; its buffers hold that step's coefficients "
                               "(one EdgePlan serves one step at a time)")
        z, = ctx.saved_tensors
        return dev.edge_loss_grad(z, ctx.plan, "given", given=ctx.plan.coef * g), None, None, None


class _EdgeBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, plan, activation, w, want_scores):
        plan.step += 1
        ctx.plan, ctx.step, ctx.d = plan, plan.step, z.shape[1]
        # the logits are written only when asked for (E scattered 4-byte stores), the coefficients never: they live in registers
        dev.edge_loss_grad(z, plan, activation, w=w, dz=plan.dz_rows(z.shape[1]), score=plan.score if want_scores else None)
        loss = (plan.piece_loss.double().sum() * w).to(torch.float32)
        if not want_scores:
            return loss, None
        ctx.mark_non_differentiable(plan.score)
        return loss, plan.score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gs):
        if ctx.plan.step != ctx.step:
            raise RuntimeError("edge_bce_loss: the plan ran another step since this forward; its buffers hold that step's gradient "
                               "(one EdgePlan serves one step at a time)")
        return ctx.plan.dz_rows(ctx.d) * g, None, None, None, None


# edge_bce_loss's default path.  Measured interleaved at the products shape, d = 100 (profiles/edge_loss.log): the fused launch 4.07 ms,
# plan reuse without fusing 3.48 ms per step -- the fused kernel stays, tested and selectable, and is not the default
FUSED_EDGE_LOSS = False


def edge_bce_loss(z, plan, activation="sigmoid", reduction="mean", return_scores=False, fused=None):
    """The training loss of the reference's link prediction on a prepared edge list, a float32 scalar on the device that carries
    the gradient to z -- `loss_fn(torch.sigmoid(torch.mm(z, z.t())[e0, e1]), labels)` of edge_predict_train (sgl/tasks/utils.py:281-293)
    without the N x N matrix.  With s_e = <z[u_e], z[v_e]> and y_e the plan's labels, per edge:
      activation="sigmoid"  the reference AS WRITTEN: its default loss_fn is binary_cross_entropy_with_logits, applied to the sigmoid
                            of the logits -- p = sigmoid(s), L = (1 - y) p + log1p(exp(-p))
      activation="none"     the with-logits loss on the logits themselves: L = max(s, 0) - s y + log1p(exp(-|s|))
    reduction "mean" (w = 1 / E) or "sum" (w = 1); the loss is w times the float64 sum of the pieces' float32 sums.
    With grad enabled and z.requires_grad there are two paths over the plan, neither of which sorts anything or uses atomics (two
    runs are bit-equal):
      fused=True   ONE launch (sgl_edge_loss_grad_f32) computes scores, loss and dZ into the plan's buffers, and the backward returns
                   the upstream gradient times that dZ; nothing but that product is allocated per step
      fused=False  plan reuse WITHOUT fusing, THE DEFAULT: device.edge_dot into the plan's score buffer, loss and coefficients by the
                   kernel's formulas in torch on E floats (a few E-sized temporaries), and in the backward one GIVEN-mode launch
                   over the plan with g x coefficients; that launch writes a NEW [n, d] dZ every step, which autograd owns
    fused=None takes FUSED_EDGE_LOSS, the faster of the two in the interleaved measurement at d = 100.  Without
    grad the scores come from device.edge_dot and the formulas run in torch on E floats.  All paths see the same logits bit for
    bit and use the same formulas for loss and coefficient (c = w (sigma(s) - y) at s = 0 too: nothing goes through the
    subgradients of max or abs); the torch evaluation may differ from the kernel's in the last bits (torch's exp / log1p are not
    the device library's, and it sums the E terms in another order).
    return_scores=True: (loss, logits [E]) -- the logits are the plan's buffer, valid until the next step.  bf16 z is refused."""
    if activation not in ("sigmoid", "none"):
        raise ValueError("edge_bce_loss: activation must be 'sigmoid' or 'none'")
    if reduction not in ("mean", "sum"):
        raise ValueError("edge_bce_loss: reduction must be 'mean' or 'sum'")
    if not isinstance(plan, EdgePlan):
        raise TypeError("edge_bce_loss: plan must be an EdgePlan")
    dev._no_bf16("edge_bce_loss", z)
    dev._check_mat(z, "z")
    plan._check_z(z, "edge_bce_loss")
    w = 1.0 / plan.n_edges if (reduction == "mean" and plan.n_edges) else 1.0
    if torch.is_grad_enabled() and z.requires_grad:
        if plan.n_edges == 0 or z.shape[1] == 0:        # nothing to launch: the torch formulas on E (or no) floats carry a zero gradient
            with torch.no_grad():
                scores = edge_scores(z, plan.edges)
                loss = _loss_of(scores, plan, activation, w)
            loss = _ZeroGrad.apply(z, loss)
        elif FUSED_EDGE_LOSS if fused is None else fused:
            loss, scores = _EdgeBCE.apply(z, plan, activation, w, bool(return_scores))
        else:
            loss, scores = _EdgeBCEUnfused.apply(z, plan, activation, w)
    else:
        with torch.no_grad():
            scores = edge_scores(z, plan.edges)
            loss = _loss_of(scores, plan, activation, w)
    return (loss, scores) if return_scores else loss


def _model_output(model, nodes, device):
    return model.model_forward(nodes, device) if hasattr(model, "model_forward") else model(nodes)


def edge_predict_train(model, train_nodes, plan, optimizer, threshold=0.5, activation="sigmoid"):
    """edge_predict_train of the reference (sgl/tasks/utils.py:274-303), full batch: one optimizer step on the plan's edges and
    (loss, roc_auc, avg_prec) of the training edges.  As there, the two metrics are taken on the THRESHOLDED predictions
    `sigmoid(s) > threshold` (0 / 1 scores: binary_ranking_metrics is tie-aware, so they are sklearn's values).  optimizer=None is
    the reference's with_params=False: the loss and metrics alone."""
    device = plan.device
    if optimizer is not None:
        model.train()
        optimizer.zero_grad()
        z = _model_output(model, train_nodes, device)
        loss, scores = edge_bce_loss(z, plan, activation=activation, return_scores=True)
        loss.backward()
        optimizer.step()
    else:
        with torch.no_grad():
            z = _model_output(model, train_nodes, device)
            loss, scores = edge_bce_loss(z, plan, activation=activation, return_scores=True)
    with torch.no_grad():
        pred = (torch.sigmoid(scores) > threshold).to(torch.float64)
        roc_auc, avg_prec = binary_ranking_metrics(pred, plan.labels)
    return float(loss.detach()), roc_auc, avg_prec


@torch.no_grad()
def edge_predict_eval(model, train_nodes, val_pos, val_neg, test_pos, test_neg, device="cuda"):
    """edge_predict_eval of the reference (sgl/tasks/utils.py:306-315): (roc_auc_val, avg_prec_val, roc_auc_test, avg_prec_test) of
    the model's output in eval mode, on the sigmoid scores as edge_predict_score ranks them"""
    model.eval()
    z = _model_output(model, train_nodes, _indexed(device))
    return edge_predict_score(z, val_pos, val_neg) + edge_predict_score(z, test_pos, test_neg)


GAELinkPredictionResult = namedtuple("GAELinkPredictionResult", ["test_roc_auc", "test_avg_prec", "history", "split"])
GAELinkPredictionResult.__doc__ = """gae_link_prediction's result: the pair LinkPredictionGAE keeps (the test scores at the best validation
scores), history = one dict per epoch (loss, roc_auc_train, avg_prec_train, roc_auc_val, avg_prec_val, roc_auc_test, avg_prec_test)
followed by the post-processing entry (epoch = "post"), and the EdgeSplit that was used"""


def gae_link_prediction(model, adj_or_split, x, epochs, lr, weight_decay, seed=42, threshold=0.5, activation="sigmoid", device="cuda"):
    """LinkPredictionGAE of the reference (sgl/tasks/link_prediction.py:14-157: __init__ and _execute), full batch, on the device.
    adj_or_split: an adjacency (scipy or DeviceAdjacency; split by mask_test_edges(adj, seed)) or an EdgeSplit.  model: a module with
    preprocess(adj_train, x) and model_forward(nodes, device) -- and optionally postprocess(adj_train, z) -- like the reference's
    BaseSGAPModel.  Adam(lr, weight_decay) when the model has parameters; per epoch edge_predict_train on the training edges and
    their negatives (ONE EdgePlan for all epochs) and edge_predict_eval; the test scores are kept where the validation scores are
    strictly the best so far (lines 120-134, bests start at 0).  The post-processing step keeps its quirk: the test edges are scored
    against ALL negative edges (train, val and test; line 156).  The mini-batch mode of the reference is not offered: it bounds
    nothing there (it still forms N x N), and per-edge scores make the full batch cheap."""
    device = _indexed(device)
    split = adj_or_split if isinstance(adj_or_split, EdgeSplit) else mask_test_edges(adj_or_split, seed=seed, device=device)
    n = int(x.shape[0])
    torch.manual_seed(seed)
    model.preprocess(split.adj_train, x)
    model = model.to(device)
    params = list(model.parameters())
    optimizer = torch.optim.Adam(params, lr=lr, weight_decay=weight_decay) if params else None
    nodes = torch.arange(n, dtype=torch.int64, device=device)
    plan = EdgePlan.from_pos_neg(split.train_edges, split.train_edges_false, n, device=device)
    best_val = [0., 0.]
    best_test = [0., 0.]
    history = []

    def keep(roc_auc_val, avg_prec_val, roc_auc_test, avg_prec_test):
        if roc_auc_val > best_val[0]:
            best_val[0], best_test[0] = roc_auc_val, roc_auc_test
        if avg_prec_val > best_val[1]:
            best_val[1], best_test[1] = avg_prec_val, avg_prec_test

    for epoch in range(epochs):
        loss, roc_auc_train, avg_prec_train = edge_predict_train(model, nodes, plan, optimizer, threshold, activation)
        scores = edge_predict_eval(model, nodes, split.val_edges, split.val_edges_false, split.test_edges, split.test_edges_false, device)
        history.append(dict(epoch=epoch, loss=loss, roc_auc_train=roc_auc_train, avg_prec_train=avg_prec_train, roc_auc_val=scores[0],
                            avg_prec_val=scores[1], roc_auc_test=scores[2], avg_prec_test=scores[3]))
        keep(*scores)
    with torch.no_grad():                              # _postprocess (lines 142-157)
        model.eval()
        z = _model_output(model, nodes, device)
        if hasattr(model, "postprocess"):
            z = model.postprocess(split.adj_train, z)
        all_neg = torch.cat((split.train_edges_false, split.val_edges_false, split.test_edges_false))
        scores = edge_predict_score(z, split.val_edges, split.val_edges_false) + edge_predict_score(z, split.test_edges, all_neg)
    history.append(dict(epoch="post", roc_auc_val=scores[0], avg_prec_val=scores[1], roc_auc_test=scores[2], avg_prec_test=scores[3]))
    keep(*scores)
    return GAELinkPredictionResult(best_test[0], best_test[1], history, split)

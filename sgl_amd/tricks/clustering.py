"""Node clustering from node features, on the MI355X: k-means and the three scores that end the NAFS clustering task.

Reference: NodeClusteringNAFS (sgl/tasks/node_clustering.py:121-258) ends every hop count with

    kmeans = KMeans(n_clusters=..., n_init=20, random_state=seed); y_pred = kmeans.fit_predict(input_features.numpy())   (254-255)
    acc, nmi, adjscore = clustering_metrics(labels, y_pred).evaluationClusterModelFromLabel()                             (256-257)

on CPU cores, after copying [N, d] to the host.  Here the features stay where nafs_ensemble_sweep left them:

  * the assignment step is one kernel (device.kmeans_assign -> sgl_kmeans_assign_f32: direct squared differences, centres in LDS);
  * the centre update needs no kernel of its own and no atomics: the per-cluster sums are M X with M the k x N membership matrix, so
    the (label, row, 1) triplets become a CSR matrix (sgl_coo_to_csr) and the library's SpMM does the rest, as the backward of the
    edge scores does (link_prediction._grad_spmm) -- deterministic like every product it computes; the counts are the differences of
    M's row pointers;
  * the three scores are functions of the k x k contingency table: one integer bincount on the device the labels are on, float64
    arithmetic on the table.

What is and is not sklearn parity: the Lloyd loop follows sklearn's stopping rule exactly, so from the SAME initial centres it ends
with the same labels after the same number of iterations wherever no row sits on a tie.  The seeding is plain k-means++ (one
candidate per step) from a torch.Generator -- sklearn's greedy variant tries 2 + ln k candidates per step and draws from numpy --
so with a seed alone the two agree only on inputs with a single optimum.

The TRAINABLE task, NodeClustering (sgl/tasks/node_clustering.py:12-119), trains a model on cluster_loss (sgl/tasks/utils.py:101-113)
with a k-means of the model output in every step (clustering_train, 116-136).  Here the output never leaves the device: kmeans above,
then ONE launch for the loss and its gradient (device.cluster_loss_grad -> sgl_cluster_loss_grad_f32), then clustering_scores:
cluster_loss, clustering_train and node_clustering below."""
from collections import namedtuple

import numpy as np
import torch

from .. import device as dev
from .nafs_features import nafs_ensemble_sweep

__all__ = ["kmeans", "KMeansResult", "clustering_scores", "nafs_node_clustering", "NodeClusteringResult",
           "cluster_loss", "clustering_train", "node_clustering", "NodeClusteringTrainResult"]

KMeansResult = namedtuple("KMeansResult", ["labels", "centres", "inertia", "n_iter"])
KMeansResult.__doc__ = """kmeans' result: labels int64 [n] and centres float32 [k, d] on x's device, inertia (float: the float64 sum of the
squared distances to the assigned centres), n_iter (sklearn's n_iter_ of the winning run)"""

_VAR_ROWS = 1 << 18      # rows per float64 slice of the variance pass


def _mean_variance(x):
    """mean over the columns of var(x, axis=0) in float64 (numpy's np.var: divisor n), in row slices so that no float64 copy of
    the whole matrix exists"""
    n, d = x.shape
    total = torch.zeros(d, dtype=torch.float64, device=x.device)
    for lo in range(0, n, _VAR_ROWS):
        total += x[lo:lo + _VAR_ROWS].sum(dim=0, dtype=torch.float64)
    mean = total / n
    sq = torch.zeros(d, dtype=torch.float64, device=x.device)
    for lo in range(0, n, _VAR_ROWS):
        sq += ((x[lo:lo + _VAR_ROWS].to(torch.float64) - mean) ** 2).sum(dim=0)
    return float((sq / n).mean()) if d else 0.0


class _Update:
    """the centre update of one matrix x: centres = (M x) / counts, M the k x n membership matrix of the labels"""

    def __init__(self, x, k):
        n = x.shape[0]
        self.x, self.k = x, k
        self.rows = torch.arange(n, dtype=torch.int64, device=x.device)
        self.ones = torch.ones(n, dtype=torch.float32, device=x.device)

    def sums(self, labels):
        from ..io import coo_to_csr_device
        m = coo_to_csr_device(labels, self.rows, self.ones, self.k, device=self.x.device, num_col=self.x.shape[0])
        return dev.DeviceCSR(m.rowptr, m.col, m.val, m.shape).spmm(self.x), m.rowptr[1:] - m.rowptr[:-1]

    def __call__(self, labels, mindist):
        sums, counts = self.sums(labels)
        if int(counts.min()) == 0:
            # An empty cluster takes the row with the largest distance to its centre (the lowest index on ties), which leaves its
            # former cluster; several empty clusters take rows in descending order of distance.  The only row of a cluster stays.
            labels = labels.clone()
            while True:
                empty = torch.nonzero(counts == 0).reshape(-1)
                if empty.numel() == 0:
                    break
                far = torch.where(torch.isnan(mindist) | (counts[labels] <= 1), torch.full_like(mindist, -1.0), mindist)
                order = torch.sort(far, descending=True, stable=True).indices[:empty.numel()]
                labels[order] = empty
                mindist = mindist.clone()
                mindist[order] = 0.0
                sums, counts = self.sums(labels)
        return sums / counts.to(torch.float32)[:, None]


def _lloyd(x, centres, update, max_iter, tol_abs):
    """sklearn's _kmeans_single_lloyd (sklearn/cluster/_kmeans.py): assign, update, stop when the labels equal the previous
    iteration's, else when the summed squared centre shift is <= tol_abs; after a stop by shift (or by max_iter) assign once more so
    that the labels belong to the returned centres"""
    labels_old, strict, n_iter = None, False, 0
    labels = mindist = None
    for it in range(max_iter):
        labels, mindist = dev.kmeans_assign(x, centres)
        new = update(labels, mindist)
        shift = float(((new.to(torch.float64) - centres.to(torch.float64)) ** 2).sum())
        centres, n_iter = new, it + 1
        if labels_old is not None and torch.equal(labels, labels_old):
            strict = True
            break
        if shift <= tol_abs:
            break
        labels_old = labels
    if not strict:
        labels, mindist = dev.kmeans_assign(x, centres)
    return KMeansResult(labels, centres, float(mindist.sum(dtype=torch.float64)), n_iter)


def _seed_plus_plus(x, k, gen):
    """plain k-means++: the first centre a uniform draw, every further one a single draw with probability proportional to the squared
    distance to the nearest centre chosen so far.  That running minimum is kept by one assignment against the NEWEST centre alone
    and torch.minimum: k reads of x, not k^2 / 2."""
    n = x.shape[0]
    draws = torch.rand(k, generator=gen, dtype=torch.float64).to(x.device)
    last = n - 1
    idx = torch.clamp((draws[0:1] * n).to(torch.int64), max=last)
    centres = torch.empty((k, x.shape[1]), dtype=torch.float32, device=x.device)
    centres[0:1] = x[idx]
    near = dev.kmeans_assign(x, centres[0:1])[1]
    for j in range(1, k):
        cum = torch.cumsum(near.to(torch.float64), 0)
        idx = torch.clamp(torch.searchsorted(cum, draws[j:j + 1] * cum[-1], right=True), max=last)
        centres[j:j + 1] = x[idx]
        near = torch.minimum(near, dev.kmeans_assign(x, centres[j:j + 1])[1])
    return centres


@torch.no_grad()
def kmeans(x, n_clusters, n_init=20, max_iter=300, tol=1e-4, seed=None, init="k-means++"):
    """Lloyd's k-means of the rows of x ([n, d] float32 CUDA tensor; an ndarray or host tensor is uploaded to the current device) on
    the device; returns a KMeansResult on x's device.

    The loop is sklearn's (KMeans(algorithm="lloyd"), _kmeans_single_lloyd): stop when the labels equal the previous iteration's,
    else when the summed squared centre shift is at most tol * mean over the columns of var(x) (float64, taken once); after a stop by
    shift one more assignment; n_iter counts as n_iter_ does; inertia is the float64 sum of the float32 squared distances.  Of n_init
    runs the lowest inertia wins, the earliest run on a tie.
    init: "k-means++", or a [k, d] tensor / array of initial centres, which forces one run.  The seeding is PLAIN k-means++, one
    candidate per step (sklearn's greedy variant tries 2 + ln k candidates per step), with draws from a torch.Generator seeded with
    `seed` (None: a fresh random seed): same seed, same device, same input give a bit-equal result -- nothing here uses atomics.
    An empty cluster takes the row with the largest distance to its centre (the lowest index on ties), which leaves its former
    cluster; several empty clusters take rows in descending order of distance (a property of this function, not sklearn parity)."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
    if not x.is_cuda:
        x = x.to("cuda")
    dev._no_bf16("kmeans", x)
    dev._check_mat(x, "x")
    n, d = x.shape
    k = int(n_clusters)
    if k < 1 or n < k:
        raise ValueError(f"n_samples={n} should be >= n_clusters={k} >= 1")
    if max_iter < 1 or n_init < 1:
        raise ValueError("max_iter and n_init must be at least 1")
    given = None
    if not isinstance(init, str):
        given = torch.as_tensor(np.asarray(init) if not torch.is_tensor(init) else init).to(device=x.device, dtype=torch.float32).contiguous()
        if given.shape != (k, d):
            raise ValueError(f"init must be [{k}, {d}]")
        n_init = 1
    elif init != "k-means++":
        raise ValueError("init must be 'k-means++' or a [k, d] matrix of centres")
    gen = torch.Generator()
    if seed is None:
        gen.seed()
    else:
        gen.manual_seed(int(seed))
    tol_abs = tol * _mean_variance(x)
    update = _Update(x, k)
    best = None
    for _ in range(n_init):
        run = _lloyd(x, given if given is not None else _seed_plus_plus(x, k, gen), update, max_iter, tol_abs)
        if best is None or run.inertia < best.inertia:
            best = run
    return best


def _table(labels_true, labels_pred):
    """the contingency table of two labelings as an int64 ndarray [distinct true, distinct predicted]: one bincount on their device"""
    t, p = (torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).reshape(-1) for v in (labels_true, labels_pred))
    if t.numel() != p.numel():
        raise ValueError("labels_true and labels_pred must have the same length")
    where = t.device if t.is_cuda else p.device
    t, p = t.to(where), p.to(where)
    (ut, it), (up, ip) = (torch.unique(v, return_inverse=True) for v in (t, p))
    kt, kp = int(ut.numel()), int(up.numel())
    return torch.bincount(it * kp + ip, minlength=kt * kp).reshape(kt, kp).cpu().numpy().astype(np.int64)


def _entropy(counts, n):
    c = counts[counts > 0].astype(np.float64)
    return 0.0 if c.size <= 1 else float(-np.sum((c / n) * (np.log(c) - np.log(n))))


def clustering_scores(labels_true, labels_pred):
    """(acc, nmi, adjscore): the three values of clustering_metrics.evaluationClusterModelFromLabel (sgl/tasks/clustering_metrics.py:
    61-66) -- sklearn's normalized_mutual_info_score (arithmetic-mean normalisation) and adjusted_rand_score, and the accuracy under
    the best one-to-one matching of predicted clusters to classes -- from the contingency table: one integer bincount on the device
    the labels are on (CPU included), float64 on the k x k table after it.  The matching is scipy's linear_sum_assignment where the
    reference uses Munkres: the matched COUNT is unique even where the matching is not, so the two agree.
    Difference from the reference: when the numbers of distinct true and predicted labels differ its clusteringAcc returns a bare 0
    and its caller fails to unpack it; here acc is 0.0 and nmi and adjscore are returned all the same."""
    from scipy.optimize import linear_sum_assignment
    table = _table(labels_true, labels_pred)
    n = int(table.sum())
    kt, kp = table.shape
    a, b = table.sum(1), table.sum(0)
    # normalized mutual information
    if kt == kp and kt <= 1:
        nmi = 1.0
    elif kt == 1 or kp == 1:
        nmi = 0.0
    else:
        i, j = np.nonzero(table)
        nij = table[i, j].astype(np.float64)
        terms = (nij / n) * (np.log(nij) - np.log(n)) + (nij / n) * (-np.log((a[i] * b[j]).astype(np.float64)) + 2.0 * np.log(n))
        terms = np.where(np.abs(terms) < np.finfo(np.float64).eps, 0.0, terms)
        mi = max(float(terms.sum()), 0.0)
        nmi = 0.0 if mi == 0 else mi / (0.5 * (_entropy(a, n) + _entropy(b, n)))
    # adjusted Rand index from the pair counts, in Python integers
    sq = int((table.astype(object) ** 2).sum()) if table.size else 0
    sa, sb = int((a.astype(object) ** 2).sum()), int((b.astype(object) ** 2).sum())
    tp = sq - n
    fp, fn = sb - sq, sa - sq
    tn = n * n - tp - fp - fn - n
    if fn == 0 and fp == 0:
        adjscore = 1.0
    else:
        adjscore = 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    # accuracy under the best one-to-one matching
    if kt != kp or n == 0:
        acc = 0.0
    else:
        rows, cols = linear_sum_assignment(-table)
        acc = float(int(table[rows, cols].sum()) / n)
    return acc, float(nmi), float(adjscore)


NodeClusteringResult = namedtuple("NodeClusteringResult", ["metrics", "best_hop_acc", "best_hop_nmi", "best_hop_adjscore", "acc", "nmi",
                                                           "adjscore"])
NodeClusteringResult.__doc__ = """nafs_node_clustering's result: metrics = {hop count: (acc, nmi, adjscore)} and the six values
NodeClusteringNAFS keeps (best_hop_acc, best_hop_nmi, best_hop_adjscore, acc, nmi, adjscore)"""


@torch.no_grad()
def nafs_node_clustering(adj, x, y, hops, r_list=(0.5, 0.4, 0.3, 0.2, 0.1, 0), method="mean", n_init=20, seed=42, device="cuda",
                         strict_order=False, reorder=None):
    """NodeClusteringNAFS._execute (sgl/tasks/node_clustering.py:171-258): for every hop count of `hops` (an int = range(hops), or a
    list) the NAFS ensemble features, their k-means labels (k = the number of distinct labels in y, n_init runs seeded with `seed`)
    and (acc, nmi, adjscore) against y; then the best-hop bookkeeping of lines 189-197 (strictly greater wins, the bests start at
    0).  One nafs_ensemble_sweep -- one propagation per r for ALL hop counts -- whose consumer clusters and scores each feature matrix
    as soon as its ensemble is complete; only three floats per hop count outlive it.  Returns a NodeClusteringResult."""
    device = torch.device(device)
    y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).reshape(-1).to(device)
    k = int(torch.unique(y).numel())

    def cluster(hop, feats):
        return clustering_scores(y, kmeans(feats, k, n_init=n_init, seed=seed).labels)

    metrics = nafs_ensemble_sweep(adj, x, hops, r_list=r_list, method=method, device=device, strict_order=strict_order, reorder=reorder,
                                  consume=cluster)
    best_acc, best_nmi, best_adjscore = 0., 0., 0.
    best_hop_acc, best_hop_nmi, best_hop_adjscore = 0, 0, 0
    for hop in (range(hops) if isinstance(hops, int) else hops):
        acc, nmi, adjscore = metrics[int(hop)]
        if acc > best_acc:
            best_acc, best_hop_acc = acc, hop
        if nmi > best_nmi:
            best_nmi, best_hop_nmi = nmi, hop
        if adjscore > best_adjscore:
            best_adjscore, best_hop_adjscore = adjscore, hop
    return NodeClusteringResult(metrics, best_hop_acc, best_hop_nmi, best_hop_adjscore, best_acc, best_nmi, best_adjscore)


# ---- the trainable task ---------------------------------------------------------------------------------------------------------------------
class _ClusterLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, labels, centres, w):
        dx, row_loss = dev.cluster_loss_grad(output, centres, labels, w, dx=True, row_loss=True)
        ctx.dx = dx
        return (row_loss.sum(dtype=torch.float64) * w).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dx, ctx.dx = ctx.dx, None
        if dx is None:
            raise RuntimeError("cluster_loss: backward ran twice; the gradient buffer of the forward launch was handed out the first time")
        return dx.mul_(g), None, None, None


def _device_labels(labels, k, n, device, check):
    """int64 [n] on `device`; check=True: labels in [-k, k) wrap as numpy indices do, anything else raises IndexError (one host
    read of the two extremes); check=False: taken as they are (labels that come from kmeans)"""
    t = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels)
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
        raise TypeError("cluster_loss: labels must be integers")
    t = t.reshape(-1).to(device=device, dtype=torch.int64).contiguous()
    if t.numel() != n:
        raise ValueError(f"cluster_loss: {t.numel()} labels for {n} rows")
    if check and n:
        lo, hi = (int(v) for v in torch.aminmax(t))
        if lo < -k or hi >= k:
            raise IndexError(f"cluster_loss: label {lo if lo < -k else hi} is out of bounds for {k} centres")
        if lo < 0:
            t = torch.where(t < 0, t + k, t)
    return t


def cluster_loss(output, labels, centres, reduction="mean", check=True):
    """cluster_loss of the reference (sgl/tasks/utils.py:101-113) as a float32 scalar on the device that carries the gradient to
    `output` alone: with D_ij = |output[i] - centres[j]|_2,

        loss = (1 / n) sum_i (2 D_{i, labels[i]} - (1 / k) sum_j D_ij)        ("mean", the reference; "sum": without the 1 / n)

    output: [n, d] float32 CUDA matrix; centres: [k, d] (tensor or ndarray; moved to output's device; no gradient, as in the
    reference, which builds them from numpy); labels: n integers (tensor or ndarray).  check=True: labels in [-k, k) wrap as numpy
    indices do (dist[j, x] in the reference), anything else raises IndexError -- one host read; check=False validates nothing (for
    labels that come from kmeans): a label outside [0, k) then means "no assigned centre".
    ONE launch (sgl_cluster_loss_grad_f32) computes the per-row losses and, when output requires grad, dX as well -- the direct form,
    differences first, one read of output and one write of dX; the loss is the float64 sum of the rows' float32 losses.  The
    backward multiplies that buffer by the upstream gradient in place: no launch of ours, no host synchronisation, nothing allocated.
    The gradient where a row coincides with a centre is 0 for that term (torch.norm's subgradient).  No atomics: two runs are
    bit-equal.  bf16 output is refused."""
    if reduction not in ("mean", "sum"):
        raise ValueError("cluster_loss: reduction must be 'mean' or 'sum'")
    dev._no_bf16("cluster_loss", output, centres)
    dev._check_mat(output, "output")
    if not torch.is_tensor(centres):
        centres = torch.as_tensor(np.asarray(centres), dtype=torch.float32)
    centres = centres.detach().to(device=output.device)
    dev._check_mat(centres, "centres")
    n, d = output.shape
    k = centres.shape[0]
    if k < 1 or centres.shape[1] != d:
        raise ValueError(f"cluster_loss: centres must be [k >= 1, {d}]")
    labels = _device_labels(labels, k, n, output.device, check)
    w = 1.0 / n if (reduction == "mean" and n) else 1.0
    if torch.is_grad_enabled() and output.requires_grad:
        return _ClusterLoss.apply(output, labels, centres, w)
    _, row_loss = dev.cluster_loss_grad(output.detach(), centres, labels, w, row_loss=True)
    return (row_loss.sum(dtype=torch.float64) * w).to(torch.float32)


def _model_output(model, nodes, device):
    return model.model_forward(nodes, device) if hasattr(model, "model_forward") else model(nodes)


def clustering_train(model, train_idx, y, optimizer, n_clusters, n_init=20, seed=None, device="cuda"):
    """clustering_train of the reference (sgl/tasks/utils.py:116-136), one step: model_forward, k-means of the DETACHED output
    (kmeans above: n_init runs seeded with `seed`, on the device -- the reference copies the output to the host for sklearn),
    cluster_loss on its labels and centres, backward, optimizer.step, and the three scores of the k-means labels against y.
    Returns (loss, acc, nmi, adjscore).  optimizer=None: the loss and scores alone, nothing is updated."""
    device = torch.device(device)
    if optimizer is not None:
        model.train()
        optimizer.zero_grad()
    with torch.set_grad_enabled(optimizer is not None):
        out = _model_output(model, train_idx, device)
        km = kmeans(out.detach(), n_clusters, n_init=n_init, seed=seed)
        loss = cluster_loss(out, km.labels, km.centres, check=False)
        if optimizer is not None:
            loss.backward()
            optimizer.step()
    acc, nmi, adjscore = clustering_scores(y, km.labels)
    return float(loss.detach()), acc, nmi, adjscore


NodeClusteringTrainResult = namedtuple("NodeClusteringTrainResult", ["acc", "nmi", "adjscore", "history"])
NodeClusteringTrainResult.__doc__ = """node_clustering's result: the three bests NodeClustering keeps, and history = one dict per epoch (epoch,
loss, acc, nmi, adjscore) followed by the post-processing entry (epoch = "post", without a loss)"""


def node_clustering(model, adj, x, y, epochs, lr, weight_decay, n_init=20, seed=42, device="cuda"):
    """NodeClustering._execute of the reference (sgl/tasks/node_clustering.py:54-119), on the device: model.preprocess(adj, x), Adam(lr,
    weight_decay), `epochs` steps of clustering_train over ALL nodes (k = the number of distinct labels in y), then the final step --
    model_forward in eval mode -> model.postprocess(adj, output) when the model has one -> kmeans -> scores -- and the best-of
    bookkeeping of lines 84-98: strictly greater wins, the bests start at 0.  Returns a NodeClusteringTrainResult.
    Seeds: torch.manual_seed(seed) once, as the reference's set_seed; the k-means of epoch e is seeded with seed + e and the final one
    with seed + epochs (the reference leaves KMeans unseeded, so its runs differ; same seed, same result here).
    The reference calls `postprocess(outputs)` WITHOUT the adjacency, which BaseSGAPModel.postprocess(adj, output) does not accept: it
    raises at its final step.  Here adj is passed."""
    device = torch.device(device)
    y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).reshape(-1).to(device)
    n = int(y.numel())
    k = int(torch.unique(y).numel())
    torch.manual_seed(seed)
    model.preprocess(adj, x)
    model = model.to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    nodes = torch.arange(n, dtype=torch.int64, device=device)
    best = [0., 0., 0.]
    history = []

    def keep(scores):
        for i, v in enumerate(scores):
            if v > best[i]:
                best[i] = v

    for epoch in range(epochs):
        loss, acc, nmi, adjscore = clustering_train(model, nodes, y, optimizer, k, n_init=n_init, seed=seed + epoch, device=device)
        history.append(dict(epoch=epoch, loss=loss, acc=acc, nmi=nmi, adjscore=adjscore))
        keep((acc, nmi, adjscore))
    with torch.no_grad():                              # _postprocess (lines 106-119)
        model.eval()
        out = _model_output(model, nodes, device)
        if hasattr(model, "postprocess"):
            out = model.postprocess(adj, out)
        scores = clustering_scores(y, kmeans(out, k, n_init=n_init, seed=seed + epochs).labels)
    history.append(dict(epoch="post", acc=scores[0], nmi=scores[1], adjscore=scores[2]))
    keep(scores)
    return NodeClusteringTrainResult(best[0], best[1], best[2], history)

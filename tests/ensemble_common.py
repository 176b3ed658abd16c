"""Shared by test_ensemble_cpu.py and test_gpu_ensemble.py (importable without a GPU): numpy restatements of K16
(include/sgl_ensemble.h), the launch arithmetic of its weight gradient, and the error bounds that follow from both.

The aggregators, in the reference's parameter layout (sgl/models/simple_models.py:5-84); X[h][s] is the [n, d] matrix of sub-graph
s at hop h, idx the rows taken:

  per_feature  OneDimConvolution                              W[h]: [d, S]    out_h[i, f] = sum_s X[h][s][idx_i, f] W[h][f, s] / S
  shared       OneDimConvolutionWeightSharedAcrossFeatures    W[h]: [1, S]    out_h[i, f] = sum_s X[h][s][idx_i, f] W[h][0, s] / S
  fast         FastOneDimConvolution                          W: [S * H, 1]   out[i, f]   = sum_{s, h} X[h][s][idx_i, f] W[s * H + h, 0]

Bounds (u = 2^-24, T = the float64 value of the same float32 inputs):

  forward   the kernel rounds the first product, then one fma per further member, then the division: G + 1 roundings for a group of
            G members (G = S, or S * H for `fast`).  |out - T| <= (G + 2) u sum |x w| / divisor.
  backward  dW = a sum of products; every term passes through at most `roundings` rounded operations, where `roundings` follows the
            kernel's reduction shape (bwd_roundings below; an addition of an exact zero does not round).
            |dW - T| <= gamma(roundings) sum |terms| / divisor, gamma(k) = k u / (1 - k u)."""
import numpy as np

U = 2.0 ** -24
MODES = ("per_feature", "shared", "fast")

# ---- the launch arithmetic of sgl_ensemble_combine_bwd_f32 (sgl_ensemble.hip: bwd_per_block, bwd_blocks, sgl::pick_lpr) ----------------
BWD_MAX_BLOCKS, BWD_ROW_STEP, MEMBERS_IN_FLIGHT = 1024, 32, 8
MAX_GROUP, MAX_MEMBERS = 64, 256


def bwd_per_block(n_idx):
    per = -(-n_idx // BWD_MAX_BLOCKS)
    return BWD_ROW_STEP if per <= BWD_ROW_STEP else -(-per // BWD_ROW_STEP) * BWD_ROW_STEP


def bwd_blocks(n_idx):
    return -(-n_idx // bwd_per_block(n_idx))


def bwd_scratch(n_groups, group_size, n_idx, d, cs):
    if n_groups < 1 or group_size < 1 or n_idx < 1 or d < 1:
        return 4
    return bwd_blocks(n_idx) * n_groups * group_size * (-(-d // 4) * 4 if cs else 1)


def pick_lpr(d, vec):
    lanes, lpr = -(-d // vec), 8
    while lpr < lanes and lpr < 64:
        lpr *= 2
    return lpr


def _levels(n):
    """rounded levels of a balanced pairwise sum over n values that may be non-zero (adding an exact zero does not round)"""
    return 0 if n <= 1 else int(np.ceil(np.log2(n)))


def bwd_roundings(n_idx, d, cs, vec, divided):
    """The most rounded operations one term of a dW entry passes through, from the kernel's reduction shape.  Only operations on two
    values that can both be non-zero count: a sum that starts from zero, a lane without a row or a column, a block that does not
    exist add exact zeros.
      first level, a lane: one fma per row of its share of the range (the first one rounds the product), cs = 0: per column as well;
      first level, the workgroup: cs = 1 the row lanes of a column through LDS, one after the other; cs = 0 the butterfly over the
        wavefront (column lanes, then row lanes) and the pairwise sum of the four wavefronts;
      second level: a lane's chain over every 64th block, the butterfly over the lanes that had a block, then the division."""
    lpr = pick_lpr(d, vec)
    rpb = 256 // lpr
    rows_here = min(n_idx, bwd_per_block(n_idx))                     # rows of the fullest range
    rows_lane = -(-rows_here // rpb)
    row_lanes = min(rpb, rows_here)
    if cs:
        first = rows_lane + (row_lanes - 1)
    else:
        cols_lane = min(-(-d // (lpr * vec)) * vec, d)
        col_lanes = min(lpr, -(-d // vec))
        per_wave = 64 // lpr
        first = rows_lane * cols_lane + _levels(col_lanes) + _levels(min(per_wave, row_lanes)) + _levels(min(4, -(-row_lanes // per_wave)))
    blocks = bwd_blocks(n_idx)
    second = (-(-blocks // 64) - 1) + _levels(min(blocks, 64))
    return first + second + (1 if divided else 0)


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the aggregators in float64 --------------------------------------------------------------------------------------------------------
def take(x, idx):
    return x if idx is None else x[idx]


def forward_f64(mode, X, W, idx):
    """(outputs, bounds): per hop (one entry for `fast`) the float64 value of the float32 inputs and the forward bound"""
    H, S = len(X), len(X[0])
    outs, bounds = [], []
    if mode == "fast":
        acc = mag = 0.0
        for s in range(S):
            for h in range(H):
                p = take(X[h][s], idx).astype(np.float64) * np.float64(W[s * H + h, 0])
                acc, mag = acc + p, mag + np.abs(p)
        return [acc], [(S * H + 2) * U * mag]
    for h in range(H):
        acc = mag = 0.0
        for s in range(S):
            w = W[h][:, s].astype(np.float64)[None, :] if mode == "per_feature" else np.float64(W[h][0, s])
            p = take(X[h][s], idx).astype(np.float64) * w
            acc, mag = acc + p, mag + np.abs(p)
        outs.append(acc / S)
        bounds.append((S + 2) * U * mag / S)
    return outs, bounds


def backward_f64(mode, X, G, idx):
    """(gradients, magnitudes) of sum_h <out_h, G[h]> with respect to the parameters, in their layout: the float64 value and the sum of
    the absolute terms (already divided), to be multiplied by gamma(bwd_roundings(...))"""
    H, S = len(X), len(X[0])
    if mode == "fast":
        dw, mag = np.zeros((S * H, 1)), np.zeros((S * H, 1))
        for s in range(S):
            for h in range(H):
                t = take(X[h][s], idx).astype(np.float64) * G[0].astype(np.float64)
                dw[s * H + h, 0], mag[s * H + h, 0] = t.sum(), np.abs(t).sum()
        return dw, mag
    dws, mags = [], []
    for h in range(H):
        g = G[h].astype(np.float64)
        t = np.stack([take(X[h][s], idx).astype(np.float64) * g for s in range(S)], axis=-1)        # [B, d, S]
        if mode == "per_feature":
            dws.append(t.sum(axis=0) / S)
            mags.append(np.abs(t).sum(axis=0) / S)
        else:
            dws.append(t.sum(axis=(0, 1))[None, :] / S)
            mags.append(np.abs(t).sum(axis=(0, 1))[None, :] / S)
    return dws, mags


def kernel_shape(mode, S, H):
    """(n_groups, group_size, cs, divisor) of the launch an aggregator makes"""
    if mode == "fast":
        return 1, S * H, 0, 1.0
    return H, S, 1 if mode == "per_feature" else 0, float(S)


def make_weights(mode, S, H, d, rng):
    """random parameters in the reference's layout (float32)"""
    if mode == "fast":
        return rng.uniform(-1.5, 1.5, (S * H, 1)).astype(np.float32)
    shape = (d, S) if mode == "per_feature" else (1, S)
    return [rng.uniform(-1.5, 1.5, shape).astype(np.float32) for _ in range(H)]


# the shapes of the GPU tests: every width class of the lane layout (below one vector, not a multiple of 4, several chunks per lane),
# group sizes on both sides of the batch of members in flight, one and several groups, one row / under a range / several ranges
N_ROWS = 1500
WIDTHS = (1, 3, 4, 100, 147, 260)
SUBGRAPHS = (1, 2, 3, 8, 17)
HOPS = (1, 3)
BATCHES = (1, 63, 1031, None)


def make_index(B, rng, n_rows=N_ROWS):
    """B unsorted row indices with repeats and negative (from-the-end) entries; None stays None"""
    if B is None:
        return None
    idx = rng.integers(0, n_rows, B).astype(np.int64)
    if B > 2:
        idx[1] = idx[0]                                   # a repeat
        idx[B // 2] = n_rows - 1                          # the last row (the one whose tail may not be read past)
    neg = rng.random(B) < 0.3
    idx[neg] -= n_rows                                    # the same rows, counted from the end
    if B > 2:
        idx[2] = -n_rows                                  # the most negative legal index
    return idx


# ---- G23 (tests/golden/make_g23_hetero.py): the generated heterogeneous graph and the reference's recorded results -----------------------
G23_NODE_TYPES = ["paper", "author", "venue"]
G23_EDGE_TYPES = ["paper__to__author", "author__to__paper", "paper__to__paper", "paper__to__venue", "author__to__venue"]
G23_PREDICT = "paper"
G23_MODEL = dict(prop_steps=2, feat_dim=12, output_dim=3, hidden_dim=16, num_layers=2)


def g23_graph_args(g):
    """the HeteroGraph constructor arguments recorded in G23 (numpy arrays)"""
    num = {t: int(g[f"graph|x|{t}"].shape[0]) for t in G23_NODE_TYPES}
    rows = {e: g[f"graph|row|{e}"] for e in G23_EDGE_TYPES}
    cols = {e: g[f"graph|col|{e}"] for e in G23_EDGE_TYPES}
    weights = {e: np.ones(len(rows[e]), np.float32) for e in G23_EDGE_TYPES}
    return dict(row_dict=rows, col_dict=cols, edge_weight_dict=weights, num_node_dict=num, node_types=list(G23_NODE_TYPES),
                edge_types=list(G23_EDGE_TYPES), node_id_dict=None, x_dict={t: g[f"graph|x|{t}"] for t in G23_NODE_TYPES},
                y_dict={G23_PREDICT: g["graph|y"]})


def g23_samples(g):
    k = 0
    while f"sample|{k}|types" in g:
        yield k, [str(t) for t in g[f"sample|{k}|types"]], bool(g[f"sample|{k}|undirected"])
        k += 1


def sample_by_edge_type_numpy(args, edge_types, undirected=True):
    """(rowptr, col, val, X, node_id) of the relation sub-graph, restated with numpy and scipy: the node types the edge types touch in
    node_types order, local ids, the mirror of an edge type whose ends differ in type, one COO -> CSR, every stored value 1"""
    import scipy.sparse as sp
    touched = {t for e in edge_types for t in (e.split("__")[0], e.split("__")[2])}
    offset, local, count, n = {}, {}, 0, 0
    for t in args["node_types"]:
        offset[t] = count
        count += args["num_node_dict"][t]
    xs, ids = [], []
    for t in args["node_types"]:
        if t in touched:
            local[t] = offset[t] - n
            n += args["num_node_dict"][t]
            xs.append(args["x_dict"][t])
            ids.append(np.arange(offset[t], offset[t] + args["num_node_dict"][t], dtype=np.int64))
    rows, cols = [], []
    for e in edge_types:
        src, dst = e.split("__")[0], e.split("__")[2]
        r, c = args["row_dict"][e] - local[src], args["col_dict"][e] - local[dst]
        if undirected and src != dst:
            r, c = np.concatenate((r, c)), np.concatenate((c, r))
        rows.append(r)
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    a = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int64), a.indices.astype(np.int32), np.ones(a.nnz, np.float32), np.vstack(xs), np.concatenate(ids)


def g23_aggregator(g, mode):
    """(X[h][s], parameters in the reference's layout, idx, G, recorded keys) of the aggregator record of `mode`"""
    X = g["agg|X"]
    H, S = X.shape[:2]
    keys = [str(k) for k in g[f"agg|{mode}|keys"]]
    params = [g[f"agg|{mode}|param|{k}"] for k in keys]
    W = params[0] if mode == "fast" else params
    return [[X[h, s] for s in range(S)] for h in range(H)], W, g["agg|idx"], list(g[f"agg|{mode}|G"]), keys

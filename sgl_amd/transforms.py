"""Graph transforms on the device, under the names of the reference's sgl/data/transforms.py: sub-graphs, node and edge dropping,
self-loop removal, feature masking.  The reference takes the graph back to a COO edge list, indexes it with a boolean mask and
builds a new scipy csr_matrix; here a DeviceAdjacency (a canonical CSR: columns sorted and unique inside a row) is filtered into a
new DeviceAdjacency by one stable compaction (device.csr_select -> sgl_csr_select_rowptr / sgl_csr_select_fill): no
sort, no host round trip.  A scipy matrix is uploaded first; every result lives on the device.

Masks that speak of edges are in CSR ENTRY ORDER (row by row, columns ascending -- the order of an Edge built from the canonical
CSR's COO), and no mask is ever written to.

Random draws are the library's counter hash (csrc/sgl_hash.h; stream 103 for edges, 104 for nodes), uniform, and p is the DROPPING
probability: an item is dropped iff h < T, T = floor(p 2^64).  The reference draws `torch.randn(n) >= p`, a normal deviate, so at
p = 0.5 it keeps a 0.308 share; its docstring says what is implemented here.

Deliberate differences from the reference under force_undirected:
  * the decision is taken per unordered pair and every stored direction keeps its OWN value; the reference keeps the upper triangle
    and mirrors it, which also invents a lower entry for an upper entry whose mirror was never stored (here there is none);
  * a kept self-loop keeps its value; the reference stores it twice and csr_matrix sums the two.
On a symmetric matrix with a zero diagonal the results are identical.

The transforms that ADD entries -- add_edges, add_self_loops, and to_undirected of the reference's sgl/data/utils.py -- are the
row-wise union of two canonical CSRs (device.csr_merge -> sgl_csr_merge_rowptr / sgl_csr_merge_fill): a merge of
sorted rows, no sort of the entries already stored.  Under SUM the result is bit-equal to the reference's csr_matrix of the
concatenated lists wherever a pair occurs at most twice in the concatenation; a pair that occurs three times or more is the stored
value plus the storage-order float32 sum of the added duplicates, where scipy adds in whatever order its unstable in-row sort leaves.
Deliberate difference under add_edges(del_repeated=True): the reference keeps whichever duplicate its unstable argsort puts first;
here the STORED value always wins, and among duplicates of the added list their storage-order sum stands.
delete_repeated_edges and sort_edges are not ported: a DeviceAdjacency is canonical by construction (rows sorted, pairs unique)."""
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import device as dev
from .io import DeviceAdjacency

__all__ = ["Subgraph", "get_subgraph", "random_drop_nodes", "drop_edges", "biased_drop_edges", "random_drop_edges", "remove_self_loops",
           "mask_features", "drop_threshold", "node_keep_mask", "add_edges", "add_self_loops", "to_undirected"]

Subgraph = namedtuple("Subgraph", ["adj", "x", "y", "node_ids"])      # node_ids: int64, the old ids of the kept nodes, ascending

EDGE_DROP_STREAM, NODE_DROP_STREAM = 103, 104
_P_MESSAGE = "Dropout probability has to be between 0 and 1!"
_NODE_MASK_MESSAGE = "the shape of node mask is wrong!"
_EDGE_MASK_MESSAGE = "the shape of edge drop mask is wrong!"
_ADD_SHAPE_MESSAGE = "add indices must be in shape of (2, x)!"
_ADD_RANGE_MESSAGE = "indices must be in range of [0, num_node)!"
_SELF_LOOP_MESSAGE = "add weights must be in shape of [num_node]!"


def drop_threshold(p):
    """T = floor(p 2^64), exactly, from the rational value of the float p: an item is dropped iff its 64-bit hash is below T"""
    p = float(p)
    if not 0.0 <= p <= 1.0:                       # NaN too
        raise ValueError(_P_MESSAGE)
    return int(Fraction(p) * (1 << 64))


def _adjacency(adj, device="cuda"):
    if isinstance(adj, DeviceAdjacency):
        return adj
    return DeviceAdjacency.from_scipy(adj, device=device)


def _empty(shape, device):
    return DeviceAdjacency(torch.zeros(shape[0] + 1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.int32, device=device),
                           torch.empty(0, dtype=torch.float32, device=device), shape)


def _mask(mask, size, message, device, dims=1):
    """a boolean mask of any kind as a contiguous bool tensor on `device` (a copy unless it already is one; never written)"""
    if not torch.is_tensor(mask):
        mask = torch.from_numpy(np.asarray(mask))
    if mask.dim() != dims or tuple(mask.shape) != tuple(size):
        raise ValueError(message)
    return mask.to(device=device, dtype=torch.bool).contiguous()


def _rows(t, device, dtype=None):
    if t is None:
        return None
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.asarray(t))
    return t.to(device=device, dtype=dtype) if dtype is not None else t.to(device=device)


@torch.no_grad()
def get_subgraph(adj, node_mask, keep_ids=False, x=None, y=None):
    """The nodes with node_mask[i] set and the edges among them: Subgraph(adj, x, y, node_ids).  keep_ids=False renumbers the kept
    nodes 0 .. k - 1 in their old order (scipy's a[m][:, m]), gathers x's rows (device.gather_rows) and indexes y; keep_ids=True
    keeps the shape and the ids, and zeroes the dropped rows of a COPY of x (the reference writes into g.x).  An all-false mask gives
    the graph without entries: 0 x 0, or n x n under keep_ids."""
    adj = _adjacency(adj)
    n = adj.shape[0]
    if adj.shape[1] != n:
        raise ValueError("get_subgraph: the adjacency must be square")
    dv = adj.device
    mask = _mask(node_mask, (n,), _NODE_MASK_MESSAGE, dv)
    x, y = _rows(x, dv, torch.float32), _rows(y, dv)
    node_ids = torch.nonzero(mask).reshape(-1)
    k = int(node_ids.numel())
    ids = torch.arange(n, dtype=torch.int32, device=dv) if keep_ids else (torch.cumsum(mask, 0, dtype=torch.int32) - 1)   # exclusive scan
    n_out = n if keep_ids else k
    if k == 0:
        sub = _empty((n_out, n_out), dv)
    else:
        id_map = torch.where(mask, ids, torch.full_like(ids, -1)).contiguous()
        sub = dev.csr_select(adj, row_map=id_map, col_map=id_map, n_rows_out=n_out, n_cols_out=n_out)
    if keep_ids:
        if x is not None:
            x = x.clone()
            x[~mask] = 0
    else:
        if x is not None:
            x = dev.gather_rows(x, node_ids) if k else x[:0].clone()
        if y is not None:
            y = y[mask]
    return Subgraph(sub, x, y, node_ids)


def node_keep_mask(n, p, seed=0, device="cuda"):
    """bool [n] on `device`: node i is kept iff h(seed, 104, i, 0) >= floor(p 2^64)"""
    from .tricks.link_prediction import _hash4, _u64
    t = drop_threshold(p)
    if t >> 64:
        return torch.zeros(n, dtype=torch.bool, device=device)
    h = _hash4(seed, NODE_DROP_STREAM, torch.arange(n, dtype=torch.int64, device=device), 0)
    return (h ^ _u64(1 << 63)) >= (_u64(t) ^ _u64(1 << 63))          # the top bit flipped: unsigned order as signed


@torch.no_grad()
def random_drop_nodes(adj, p=0.5, keep_ids=False, seed=0, x=None, y=None):
    """Drop every node with probability p: (Subgraph, node_mask), node_mask[i] set = node i is kept.  p = 0 hands back the input
    adjacency itself (and x, y as given)."""
    t = drop_threshold(p)
    adj = _adjacency(adj)
    if t == 0:
        n = adj.shape[0]
        return (Subgraph(adj, x, y, torch.arange(n, dtype=torch.int64, device=adj.device)),
                torch.ones(n, dtype=torch.bool, device=adj.device))
    mask = node_keep_mask(adj.shape[0], p, seed, adj.device)
    return get_subgraph(adj, mask, keep_ids=keep_ids, x=x, y=y), mask


@torch.no_grad()
def drop_edges(adj, edge_mask, force_undirected=False):
    """Keep the entries with edge_mask[p] set (CSR entry order).  force_undirected: the flag of a pair's UPPER entry (min, max)
    decides both directions, the flags of lower entries are ignored (the reference clears them -- in the caller's mask; here the mask
    is only read), and a lower entry without a stored mirror is dropped."""
    adj = _adjacency(adj)
    mask = _mask(edge_mask, (adj.nnz,), _EDGE_MASK_MESSAGE, adj.device)
    return dev.csr_select(adj, entry_keep=mask, symmetric_mask=bool(force_undirected))


def biased_drop_edges(adj, edge_mask):
    """If edge_mask[p] is False, entry p is dropped."""
    return drop_edges(adj, edge_mask)


@torch.no_grad()
def random_drop_edges(adj, p=0.5, force_undirected=True, seed=0):
    """Drop every entry with probability p -- under force_undirected every unordered pair, both directions at once: entry (i, j)
    is dropped iff h(seed, 103, i, j) < floor(p 2^64), h taken of (min, max) under force_undirected.  p = 0 returns the input
    object, p = 1 the graph without entries (no launch)."""
    t = drop_threshold(p)
    if t == 0:
        return adj
    adj = _adjacency(adj)
    if t >> 64:
        return _empty(adj.shape, adj.device)
    return dev.csr_select(adj, drop_below=t, seed=seed, symmetric=bool(force_undirected))


@torch.no_grad()
def remove_self_loops(adj):
    """Without the stored diagonal entries."""
    return dev.csr_select(_adjacency(adj), drop_self=True)


def _add_list(add_indices, add_weights, shape):
    """the [2, x] index pairs as an integer tensor and the weights as a float32 [x] tensor (ones when None), wherever they live;
    the reference's checks and messages"""
    idx = add_indices if torch.is_tensor(add_indices) else torch.from_numpy(np.asarray(add_indices))
    if idx.dim() != 2 or idx.shape[0] != 2:
        raise ValueError(_ADD_SHAPE_MESSAGE)
    x = int(idx.shape[1])
    if x == 0:
        return idx, None
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError("add_edges: add indices must be integers")
    lo, hi = torch.aminmax(idx, dim=1)             # one reduction per side
    lo, hi = lo.tolist(), hi.tolist()
    if hi[0] >= shape[0] or hi[1] >= shape[1] or lo[0] < 0 or lo[1] < 0:
        raise ValueError(_ADD_RANGE_MESSAGE)
    if add_weights is not None:
        w = add_weights if torch.is_tensor(add_weights) else torch.from_numpy(np.asarray(add_weights))
        if w.dim() != 1 or w.shape[0] != x:
            raise ValueError("add_edges: add weights must be in shape of [x]")
        add_weights = w.to(torch.float32)
    return idx, add_weights


@torch.no_grad()
def add_edges(adj, add_indices, add_weights=None, del_repeated=False):
    """The entries of `adj` and the pairs add_indices [2, x] (tensor, array or list, on the host or the device; weights default to
    ones) as one canonical adjacency.  The added list goes through the ingest (io.coo_to_csr_device: a pair repeated inside the list
    is summed in storage order) and is merged with `adj` by device.csr_merge: a pair that `adj` stores too gets the sum of the two
    values (del_repeated=False; a zero sum stays stored, as in the reference's csr_matrix) or keeps the stored value
    (del_repeated=True).  An empty list returns the input object."""
    shape = adj.shape
    idx, w = _add_list(add_indices, add_weights, shape)
    if idx.shape[1] == 0:
        return adj
    adj = _adjacency(adj)
    dv = adj.device
    if w is None:
        w = torch.ones(idx.shape[1], dtype=torch.float32, device=dv)
    from .io import coo_to_csr_device
    added = coo_to_csr_device(idx[0], idx[1], w, shape[0], device=dv, num_col=shape[1])
    return dev.csr_merge(adj, added, mode="keep" if del_repeated else "sum")


@torch.no_grad()
def add_self_loops(adj, add_weights=None):
    """`adj` plus the diagonal: add_weights [num_node] (ones when None) is ADDED to a stored diagonal entry and stored where there
    was none -- a 0.0 in add_weights becomes a stored zero, as in the reference.  The diagonal is a canonical CSR as it stands, so
    nothing is ingested."""
    n = adj.shape[0]
    if adj.shape[1] != n:
        raise ValueError("add_self_loops: the adjacency must be square")
    if add_weights is not None:
        if not torch.is_tensor(add_weights):
            add_weights = torch.from_numpy(np.asarray(add_weights))
        if add_weights.dim() != 1 or add_weights.shape[0] != n:
            raise ValueError(_SELF_LOOP_MESSAGE)
    if n == 0:
        return adj
    adj = _adjacency(adj)
    dv = adj.device
    w = torch.ones(n, dtype=torch.float32, device=dv) if add_weights is None else add_weights.to(device=dv, dtype=torch.float32).contiguous()
    eye = DeviceAdjacency(torch.arange(n + 1, dtype=torch.int64, device=dv), torch.arange(n, dtype=torch.int32, device=dv), w, (n, n))
    return dev.csr_merge(adj, eye, mode="sum")


@torch.no_grad()
def to_undirected(adj, reduce="sum"):
    """`adj` merged with its transpose (built as PreparedAdjacency.normalize builds it: rows and columns swapped through the ingest).
    reduce="sum" is the reference -- its loaders stack the list with its mirror and Edge's csr_matrix sums: a pair stored both ways
    and every diagonal entry come out DOUBLED (the weight 2.0 of dataset/ogbn.py:45).  reduce="keep" leaves every stored value as it
    is and fills in only the missing direction."""
    if reduce not in ("sum", "keep"):
        raise ValueError('to_undirected: reduce must be "sum" or "keep"')
    n = adj.shape[0]
    if adj.shape[1] != n:
        raise ValueError("to_undirected: the adjacency must be square")
    adj = _adjacency(adj)
    if adj.nnz == 0:
        return adj
    from .io import coo_to_csr_device
    dv = adj.device
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dv), adj.rowptr[1:] - adj.rowptr[:-1])
    mirror = coo_to_csr_device(adj.col.to(torch.int64), rows, adj.val, n, device=dv)
    return dev.csr_merge(adj, mirror, mode=reduce)


@torch.no_grad()
def mask_features(x, feature_mask, type=0):
    """A copy of x with the masked part zeroed: type 0 by row (feature_mask [N]), 1 by column ([f]), 2 by element ([N, f])"""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.asarray(x))
    if x.dim() != 2:
        raise ValueError("mask_features: x must be a matrix")
    if type not in (0, 1, 2):
        raise ValueError("the choice of type is 0, 1, or 2!")
    n, f = x.shape
    size = ((n,), (f,), (n, f))[type]
    mask = _mask(feature_mask, size, "dimension does not match", x.device, dims=len(size))
    x = x.clone()
    if type == 1:
        x[:, mask] = 0
    else:
        x[mask] = 0
    return x

"""HeteroNodeDataset.sample_by_meta_path on a real MI355X (sgl_amd/hetero.py over device.csr_matmul): run with `-m gpu`.

The toy graph and what the REFERENCE's sample_by_meta_path returned on it are tests/golden/g24_meta_path.npz (author 6, paper 9,
field 4 in that order; the first type of a path before, after and equal to the last one; a chain of three factors; with and
without `undirected`).  Every sample is compared with the golden and with a scipy restatement of the semantics: the product of the
edge types' 0/1 patterns in type-local ids, placed into the sub-graph over the first and the last type in the graph's order."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sgl_amd import _lib
from sgl_amd.hetero import HeteroGraph, HeteroNodeDataset

pytestmark = pytest.mark.gpu
N_SAMPLES = 10


@pytest.fixture(scope="module")
def toy(goldens):
    _lib.require_gpu()
    torch.cuda.set_device(0)
    g = goldens.npz("g24_meta_path")
    node_types, edge_types = g["graph|node_types"].tolist(), g["graph|edge_types"].tolist()
    num = dict(zip(node_types, g["graph|num"].tolist()))
    rows, cols = {e: g[f"graph|row|{e}"] for e in edge_types}, {e: g[f"graph|col|{e}"] for e in edge_types}
    graph = HeteroGraph(rows, cols, {e: np.ones(len(rows[e]), np.float32) for e in edge_types}, num, node_types, edge_types,
                        x_dict={t: g[f"graph|x|{t}"] for t in node_types}, device="cuda:0")
    return g, HeteroNodeDataset(graph), rows, cols, num, node_types


def restated(path, undirected, rows, cols, num, node_types):
    offset = {t: sum(num[u] for u in node_types[:i]) for i, t in enumerate(node_types)}
    types = path.split("__")[0::2]
    product = None
    for s, d in zip(types, types[1:]):
        e = f"{s}__to__{d}"
        factor = sp.csr_matrix((np.ones(len(rows[e])), (rows[e] - offset[s], cols[e] - offset[d])), shape=(num[s], num[d]))
        product = factor if product is None else product @ factor
    kept = [t for t in node_types if t in (types[0], types[-1])]
    place = {t: sum(num[u] for u in kept[:i]) for i, t in enumerate(kept)}
    n = sum(num[t] for t in kept)
    coo = product.tocoo()
    adj = sp.csr_matrix((np.ones(coo.nnz), (coo.row + place[types[0]], coo.col + place[types[-1]])), shape=(n, n))
    adj = adj + adj.T if undirected else adj
    adj.sort_indices()
    return adj.indptr, adj.indices


@pytest.mark.parametrize("k", range(N_SAMPLES))
def test_meta_path_against_the_reference_and_the_restatement(toy, k):
    g, ds, rows, cols, num, node_types = toy
    path, undirected = str(g[f"sample|{k}|path"]), bool(g[f"sample|{k}|undirected"])
    adj, x, node_id = ds.sample_by_meta_path(path, undirected)
    rowptr, col = restated(path, undirected, rows, cols, num, node_types)
    for want_rowptr, want_col in ((rowptr, col), (g[f"sample|{k}|rowptr"], g[f"sample|{k}|col"])):
        assert np.array_equal(adj.rowptr.cpu().numpy(), want_rowptr) and np.array_equal(adj.col.cpu().numpy(), want_col)
    assert adj.shape == (len(rowptr) - 1,) * 2 and adj.nnz > 0 and bool((adj.val == 1.0).all())
    types = path.split("__")[0::2]
    _, x_edge, id_edge = ds.sample_by_edge_type(f"{types[0]}__to__{types[-1]}") if types[0] != types[-1] else (None, ds.data[types[0]].x,
                                                                                                             torch.LongTensor(ds.data.node_id_dict[types[0]]))
    assert torch.equal(x, x_edge) and torch.equal(node_id, id_edge)
    assert np.array_equal(x.cpu().numpy(), g[f"sample|{k}|x"]) and np.array_equal(node_id.numpy(), g[f"sample|{k}|node_id"])


def test_delegation_and_refusals(toy):
    g, ds = toy[:2]
    for undirected in (True, False):
        got, want = ds.sample_by_meta_path("author__to__paper", undirected), ds.sample_by_edge_type("author__to__paper", undirected)
        assert torch.equal(got[0].rowptr, want[0].rowptr) and torch.equal(got[0].col, want[0].col) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError, match="valid edge type"):
        ds.sample_by_meta_path("author__to__paper__to__paper__to__field")        # paper__to__paper is not stored
    with pytest.raises(ValueError, match="meta path"):
        ds.sample_by_meta_path("author__to__paper__to")
    with pytest.raises(TypeError):
        ds.sample_by_meta_path(["author__to__paper__to__field"])

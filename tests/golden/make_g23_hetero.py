#!/usr/bin/env python3
"""Generate tests/golden/g23_hetero.npz by IMPORTING THE REFERENCE ITSELF (as make_g22_merge_transforms.py does).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g23_hetero.py <path of the reference checkout>

Needs the reference checkout (the directory that holds its `sgl` package); nothing of the reference travels: the fixture holds the
inputs made here and recorded outputs only.

G23: the heterogeneous family of the reference on a generated graph -- 3 node types (paper 150, author 100, venue 40), d = 12, 3
classes on the papers, 5 edge types: paper__to__author and author__to__paper (the same relation stored in both directions),
paper__to__paper (both ends of one type), paper__to__venue, author__to__venue; edge lists hold repeats.  Recorded:

    graph|...                 the constructor arguments (rows, cols, features, labels, index sets)
    sample|<k>|...            HeteroNodeDataset.sample_by_edge_type for SAMPLES[k]: canonical CSR (rowptr, col, val), the stacked
                              features, node_id
    agg|<mode>|...            the three *OneDimConvolution modules on recorded inputs (S = 3, H = 2, n = 150, B = 37): parameters,
                              float32 outputs and weight gradients of sum_h <out_h, G_h>, and the same module in .double() as truth
    model|<name>|...          NARS_SIGN and Fast_NARS_SGC_WithLearnableWeights (K = 2, hidden 16, 2 layers, 3 sub-graphs given as
                              explicit subgraph_list keys): parameters, float32 logits on a recorded idx, float64-truth logits
                              (the model in .double() on hops propagated with _construct_adj and scipy's dot)

Two breakages of the reference are shimmed HERE ONLY: sample_by_edge_type calls torch.from_numpy on what Node has already turned
into a tensor (the module gets a torch proxy whose from_numpy passes tensors through), and the package imports need the stub recipe of
SURVEY.md Appendix B (the two hetero model files are loaded by path)."""
import importlib.util
import os
import sys
import types
from unittest.mock import MagicMock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, REF)

import numpy as np
import torch

for m in ["torch_geometric", "torch_geometric.data", "torch_geometric.datasets", "torch_geometric.io", "torch_sparse", "ogb",
          "ogb.nodeproppred", "munkres", "gensim", "openbox"]:
    sys.modules.setdefault(m, MagicMock())
import sgl.dataset  # noqa: E402,F401  (first: the reference's import order)
import sgl.models.base_model  # noqa: E402,F401
import sgl.data.base_dataset as ref_dataset  # noqa: E402
from sgl.data.base_data import HeteroGraph  # noqa: E402
from sgl.models import simple_models as ref_simple  # noqa: E402


class _TorchProxy:
    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def from_numpy(x):
        return x if torch.is_tensor(x) else torch.from_numpy(x)


ref_dataset.torch = _TorchProxy()
pkg = types.ModuleType("sgl.models.hetero")
pkg.__path__ = [os.path.join(REF, "sgl", "models", "hetero")]
sys.modules["sgl.models.hetero"] = pkg


def load(name):
    spec = importlib.util.spec_from_file_location("sgl.models.hetero." + name, os.path.join(REF, "sgl", "models", "hetero", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NARS_SIGN = load("nars_sign").NARS_SIGN
FAST = load("fast_nars_sgc").Fast_NARS_SGC_WithLearnableWeights

SEED = 23
NODE_TYPES = ["paper", "author", "venue"]
NUM = {"paper": 150, "author": 100, "venue": 40}
EDGE_TYPES = ["paper__to__author", "author__to__paper", "paper__to__paper", "paper__to__venue", "author__to__venue"]
N_EDGES = {"paper__to__author": 420, "author__to__paper": 420, "paper__to__paper": 380, "paper__to__venue": 150, "author__to__venue": 160}
D, C, K, HIDDEN, LAYERS = 12, 3, 2, 16, 2
PREDICT = "paper"
SAMPLES = [(("paper__to__author",), True), (("paper__to__paper",), True), (("paper__to__author", "paper__to__venue"), True),
           (("author__to__paper", "paper__to__paper"), True), (("author__to__venue",), True), (tuple(EDGE_TYPES), True),
           (("paper__to__author", "paper__to__paper"), False)]
SUBGRAPHS = [("paper__to__author", "paper__to__paper"), ("paper__to__paper", "paper__to__venue"), ("author__to__venue", "paper__to__author")]
F = np.float32


def make_graph(rng):
    """labels on the papers, features = a class centre + noise (authors and venues: the centre of a class drawn for them), edges that
    prefer ends of one class, with repeats"""
    offsets, count = {}, 0
    for t in NODE_TYPES:
        offsets[t] = count
        count += NUM[t]
    centres = rng.standard_normal((C, D))
    klass = {t: rng.integers(0, C, NUM[t]) for t in NODE_TYPES}
    x = {t: (centres[klass[t]] + 0.8 * rng.standard_normal((NUM[t], D))).astype(F) for t in NODE_TYPES}
    rows, cols = {}, {}
    for e in EDGE_TYPES:
        src, _, dst = e.split("__")
        r = rng.integers(0, NUM[src], N_EDGES[e])
        c = rng.integers(0, NUM[dst], N_EDGES[e])
        same = np.nonzero(rng.random(N_EDGES[e]) < 0.7)[0]           # most edges join ends of one class
        for i in same:
            pool = np.nonzero(klass[dst] == klass[src][r[i]])[0]
            c[i] = pool[rng.integers(0, len(pool))]
        r[-5:], c[-5:] = r[:5], c[:5]                                # repeats
        rows[e], cols[e] = (r + offsets[src]).astype(np.int64), (c + offsets[dst]).astype(np.int64)
    rows["author__to__paper"], cols["author__to__paper"] = cols["paper__to__author"].copy(), rows["paper__to__author"].copy()
    perm = rng.permutation(NUM[PREDICT])
    return dict(rows=rows, cols=cols, x=x, y=klass[PREDICT].astype(np.int64), train=np.sort(perm[:60]), val=np.sort(perm[60:100]),
                test=np.sort(perm[100:]))


def reference_dataset(g):
    graph = HeteroGraph({e: g["rows"][e] for e in EDGE_TYPES}, {e: g["cols"][e] for e in EDGE_TYPES},
                        {e: np.ones(len(g["rows"][e]), F) for e in EDGE_TYPES}, dict(NUM), list(NODE_TYPES), list(EDGE_TYPES), None,
                        {t: g["x"][t] for t in NODE_TYPES}, {PREDICT: g["y"]})
    ds = object.__new__(ref_dataset.HeteroNodeDataset)               # (its __init__ downloads and processes files)
    ds._name, ds._data = "g23", graph
    ds._train_idx, ds._val_idx, ds._test_idx = (torch.from_numpy(g[k]) for k in ("train", "val", "test"))
    return ds


def canonical(adj):
    adj = adj.tocsr().copy()
    adj.sum_duplicates()
    adj.sort_indices()
    return adj.indptr.astype(np.int64), adj.indices.astype(np.int32), adj.data.astype(F)


def aggregator_records(out, rng):
    S, H, n, B = 3, 2, NUM[PREDICT], 37
    X = rng.standard_normal((H, S, n, D)).astype(F)
    idx = rng.integers(0, n, B).astype(np.int64)
    idx[1], idx[5] = idx[0], n - 1
    out["agg|X"], out["agg|idx"] = X, idx
    for mode, make in (("per_feature", lambda: ref_simple.OneDimConvolution(S, H, D)),
                       ("shared", lambda: ref_simple.OneDimConvolutionWeightSharedAcrossFeatures(S, H)),
                       ("fast", lambda: ref_simple.FastOneDimConvolution(S, H))):
        torch.manual_seed(SEED + len(mode))
        mod = make()
        if mode == "fast":                                           # (ones by construction: make the weights tell the members apart)
            with torch.no_grad():
                next(mod.parameters()).copy_(torch.from_numpy(rng.uniform(0.5, 1.5, (S * H, 1)).astype(F)))
        n_out = 1 if mode == "fast" else H
        G = rng.standard_normal((n_out, B, D)).astype(F)
        out[f"agg|{mode}|G"] = G
        out[f"agg|{mode}|keys"] = np.array(list(mod.state_dict().keys()))
        for k, v in mod.state_dict().items():
            out[f"agg|{mode}|param|{k}"] = v.numpy().copy()
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            m = make().to(dt)
            m.load_state_dict({k: v.to(dt) for k, v in mod.state_dict().items()})
            rows = [[torch.from_numpy(X[h, s][idx]).to(dt) for s in range(S)] for h in range(H)]
            if mode == "fast":
                feats = torch.stack([torch.stack(r, dim=2) for r in rows], dim=3)
                res = [m(feats.view(B, D, S * H))]
            else:
                res = m(rows)
            sum((o * torch.from_numpy(G[i]).to(dt)).sum() for i, o in enumerate(res)).backward()
            assert all(o.dtype == dt for o in res)
            out[f"agg|{mode}|out|{tag}"] = np.stack([o.detach().numpy() for o in res])
            for k, p in m.named_parameters():
                out[f"agg|{mode}|grad|{tag}|{k}"] = p.grad.numpy().copy()


def model_records(out, ds, g, rng):
    idx = np.sort(rng.permutation(NUM[PREDICT])[:48]).astype(np.int64)
    idx[3] = idx[2]
    out["model|idx"] = idx
    out["model|subgraphs"] = np.array(["|".join(k) for k in SUBGRAPHS])
    subgraph_list = [(key, ds.sample_by_edge_type(list(key))) for key in SUBGRAPHS]
    start = list(NODE_TYPES).index(PREDICT)
    assert start == 0
    for name, cls in (("NARS_SIGN", NARS_SIGN), ("Fast_NARS_SGC_WithLearnableWeights", FAST)):
        torch.manual_seed(SEED + len(name))
        model = cls(K, D, C, HIDDEN, LAYERS, len(SUBGRAPHS))
        with torch.no_grad():                                        # aggregator weights that tell sub-graphs and hops apart
            for p in model._aggregator.parameters():
                p.copy_(torch.from_numpy(rng.uniform(0.4, 1.6, tuple(p.shape)).astype(F)))
        out[f"model|{name}|keys"] = np.array(list(model.state_dict().keys()))
        for k, v in model.state_dict().items():
            out[f"model|{name}|param|{k}"] = v.numpy().copy()
        model.preprocess(ds, PREDICT, subgraph_list=subgraph_list)
        model.eval()
        with torch.no_grad():
            y = model.model_forward(torch.from_numpy(idx), torch.device("cpu"))
        assert y.dtype == torch.float32 and tuple(y.shape) == (len(idx), C)
        out[f"model|{name}|out"] = y.numpy().copy()
        # float64 truth: the same model in .double() on hops propagated in float64
        hops = [[] for _ in range(K + 1)]
        for key, (adj, feature, node_id) in subgraph_list:
            a = model._pre_graph_op._construct_adj(adj).astype(np.float64)
            cur = [feature.astype(np.float64)]
            for _ in range(K):
                cur.append(a.dot(cur[-1]))
            pos = list(node_id).index(ds.data.node_id_dict[PREDICT][0])
            for i, h in enumerate(cur):
                hops[i].append(torch.from_numpy(h[pos:pos + NUM[PREDICT]]))
        model = model.double()
        if name == "NARS_SIGN":
            model._propagated_feat_list_list = hops
        else:
            t = torch.stack([torch.stack(x, dim=2) for x in hops], dim=3)
            model._propagated_feat_list_list = t.view(t.shape[0], t.shape[1], t.shape[2] * t.shape[3])
        with torch.no_grad():
            y64 = model.model_forward(torch.from_numpy(idx), torch.device("cpu"))
        assert y64.dtype == torch.float64
        out[f"model|{name}|out|f64"] = y64.numpy().copy()
        print(name, "max |f32 - f64| =", float(np.abs(y.numpy() - y64.numpy()).max()))


def main():
    rng = np.random.default_rng(SEED)
    g = make_graph(rng)
    out = {"graph|y": g["y"], "graph|train": g["train"], "graph|val": g["val"], "graph|test": g["test"]}
    for e in EDGE_TYPES:
        out[f"graph|row|{e}"], out[f"graph|col|{e}"] = g["rows"][e], g["cols"][e]
    for t in NODE_TYPES:
        out[f"graph|x|{t}"] = g["x"][t]
    ds = reference_dataset(g)
    for k, (types_, undirected) in enumerate(SAMPLES):
        adj, x, node_id = ds.sample_by_edge_type(list(types_), undirected)
        rowptr, col, val = canonical(adj)
        assert np.all(val == 1.0) and x.dtype == F
        out[f"sample|{k}|types"], out[f"sample|{k}|undirected"] = np.array(list(types_)), np.array(undirected)
        out[f"sample|{k}|rowptr"], out[f"sample|{k}|col"], out[f"sample|{k}|val"] = rowptr, col, val
        out[f"sample|{k}|x"], out[f"sample|{k}|node_id"] = x, node_id.numpy().astype(np.int64)
    aggregator_records(out, rng)
    model_records(out, ds, g, rng)
    path = os.path.join(HERE, "g23_hetero.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()

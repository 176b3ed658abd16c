"""The heterogeneous family on the device against G23 (tests/golden/make_g23_hetero.py: the reference's own results on a generated
three-type graph): the relation sub-graphs bit for bit, the aggregators' outputs and weight gradients inside the derived bounds, the
two NARS models under the criteria of test_models_match_reference_goldens, a training step, and the task."""
import numpy as np
import pytest
import torch

import ensemble_common as ec
import oracle

from sgl_amd import _lib
from sgl_amd import hetero as het
from sgl_amd.models import hetero as models
from sgl_amd.models import simple_models as sm
from sgl_amd.tricks import HeteroNodeClassification, hetero_node_classification

pytestmark = pytest.mark.gpu
TOL = 1e-5                                     # the contract against the reference's float32 results


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def dataset(goldens, cuda):
    g = goldens.npz("g23_hetero")
    graph = het.HeteroGraph(**ec.g23_graph_args(g), device=cuda)
    return het.HeteroNodeDataset(graph, g["graph|train"], g["graph|val"], g["graph|test"])


def test_sample_by_edge_type_equals_the_reference_bit_for_bit(goldens, dataset, cuda):
    g = goldens.npz("g23_hetero")
    for k, types_, undirected in ec.g23_samples(g):
        adj, x, node_id = dataset.sample_by_edge_type(types_, undirected)
        assert adj.rowptr.device == cuda and x.device == cuda and adj.shape == (len(node_id), len(node_id))
        for name, got in (("rowptr", adj.rowptr), ("col", adj.col), ("val", adj.val), ("x", x), ("node_id", node_id)):
            got, want = got.cpu().numpy(), g[f"sample|{k}|{name}"]
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (k, types_, name)
    one = dataset.sample_by_edge_type("paper__to__paper")             # a single edge type may be given as a string
    assert one[0].shape == (150, 150)


@pytest.mark.parametrize("mode", ec.MODES)
def test_aggregators_match_the_recorded_truth_inside_the_bounds(goldens, cuda, mode):
    g = goldens.npz("g23_hetero")
    X, W, idx, G, keys = ec.g23_aggregator(g, mode)
    H, S, d, B = len(X), len(X[0]), X[0][0].shape[1], len(idx)
    _, _, cs, divisor = ec.kernel_shape(mode, S, H)
    mod = {"per_feature": lambda: sm.OneDimConvolution(S, H, d), "shared": lambda: sm.OneDimConvolutionWeightSharedAcrossFeatures(S, H),
           "fast": lambda: sm.FastOneDimConvolution(S, H)}[mode]()
    mod.load_state_dict({k: torch.from_numpy(g[f"agg|{mode}|param|{k}"]) for k in keys})
    mod = mod.to(cuda)
    X_d = [[torch.from_numpy(x).to(cuda) for x in row] for row in X]
    outs = mod.combine(X_d, torch.from_numpy(idx).to(cuda))
    outs = outs if isinstance(outs, list) else [outs]
    sum((o * torch.from_numpy(gg).to(cuda)).sum() for o, gg in zip(outs, G)).backward()
    T, bound = ec.forward_f64(mode, X, W, idx)
    for o, t, b, t64 in zip(outs, T, bound, g[f"agg|{mode}|out|f64"]):
        assert np.all(np.abs(o.detach().cpu().numpy().astype(np.float64) - t64) <= b)
    dT, mag = ec.backward_f64(mode, X, G, idx)
    mag = mag if isinstance(mag, list) else [mag]
    gam = ec.gamma(ec.bwd_roundings(B, d, cs, 4 if d % 4 == 0 else 1, divisor != 1.0))
    for (k, p), m in zip(mod.named_parameters(), mag):
        err = np.abs(p.grad.cpu().numpy().astype(np.float64) - g[f"agg|{mode}|grad|f64|{k}"])
        assert np.all(err <= gam * m), (k, float((err - gam * m).max()))


def subgraph_list(goldens, dataset):
    keys = [tuple(str(k).split("|")) for k in goldens.npz("g23_hetero")["model|subgraphs"]]
    return [(key, dataset.sample_by_edge_type(list(key))) for key in keys]


@pytest.mark.parametrize("name", ("NARS_SIGN", "Fast_NARS_SGC_WithLearnableWeights"))
def test_models_match_the_reference(goldens, dataset, cuda, name):
    g = goldens.npz("g23_hetero")
    model = getattr(models, name)(*ec.G23_MODEL.values(), 3)
    model.load_state_dict({str(k): torch.from_numpy(g[f"model|{name}|param|{k}"]) for k in g[f"model|{name}|keys"]})
    model = model.to(cuda).eval()
    model.preprocess(dataset, ec.G23_PREDICT, subgraph_list=subgraph_list(goldens, dataset))
    hops = model._propagated_feat_list_list
    assert len(hops) == 3 and all(len(h) == 3 and all(x.is_cuda and tuple(x.shape) == (150, 12) for x in h) for h in hops)
    idx = g["model|idx"]
    with torch.no_grad():
        y = model.model_forward(torch.from_numpy(idx), cuda)
        y_dev = model.model_forward(torch.from_numpy(idx).to(cuda), cuda)
        y_all = model.model_forward(range(150), cuda)
    # (all rows in place against gathered rows: the same aggregate; the head's GEMM over another batch size may round differently)
    assert torch.equal(y, y_dev) and torch.allclose(y_all[torch.from_numpy(idx).to(cuda)], y, rtol=1e-5, atol=1e-6)
    rep = oracle.truth_report(y.cpu().numpy(), g[f"model|{name}|out"], g[f"model|{name}|out|f64"])
    assert rep["ok"], (name, rep)
    rep = oracle.parity_report(y.cpu().numpy(), g[f"model|{name}|out"], TOL, rowwise=False)
    assert rep["ok"], (name, rep)
    # one optimiser step: every parameter gets a finite gradient, the aggregator's included
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    out = model.model_forward(g["graph|train"], cuda)
    torch.nn.functional.cross_entropy(out, torch.from_numpy(g["graph|y"][g["graph|train"]]).to(cuda)).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert all(p.grad.abs().max() > 0 for p in model._aggregator.parameters())
    opt.step()
    if name.startswith("Fast"):
        assert tuple(model.subgraph_weight.shape) == (3,)
    # a sub-graph that does not touch the predict class is skipped; the count that remains must be the model's
    extra = subgraph_list(goldens, dataset) + [(("author__to__venue",), dataset.sample_by_edge_type("author__to__venue"))]
    model.preprocess(dataset, ec.G23_PREDICT, subgraph_list=extra)
    assert len(model._propagated_feat_list_list[0]) == 3
    with pytest.raises(ValueError, match="2 of the given sub-graphs.*random_subgraph_num=3"):
        model.preprocess(dataset, ec.G23_PREDICT, subgraph_list=extra[1:])


def test_task_learns_the_generated_graph(goldens, dataset, cuda):
    g = goldens.npz("g23_hetero")
    y = g["graph|y"]
    chance = np.bincount(y[g["graph|test"]]).max() / len(g["graph|test"])
    model = models.NARS_SIGN(*ec.G23_MODEL.values(), 3)
    res = hetero_node_classification(model, dataset, ec.G23_PREDICT, epochs=40, lr=0.02, weight_decay=0.0, seed=42, random_subgraph_num=3,
                                     subgraph_edge_type_num=2, device=cuda)
    print(f"NARS_SIGN: best val {res.best_val:.3f}, test {res.best_test:.3f}, chance {chance:.3f}")
    assert len(res.history) == 40 and res.subgraph_weight is None and res.best_test > chance + 0.1
    fast = models.Fast_NARS_SGC_WithLearnableWeights(*ec.G23_MODEL.values(), 3)
    task = HeteroNodeClassification(dataset, ec.G23_PREDICT, fast, 0.02, 0.0, 40, cuda, seed=42, train_batch_size=32, eval_batch_size=64,
                                    subgraph_list=subgraph_list(goldens, dataset), record_subgraph_weight=True)
    print(f"Fast_NARS_SGC: test {task.test_acc:.3f}, sub-graph weights {task.subgraph_weight.tolist()}")
    assert task.test_acc > chance + 0.1 and tuple(task.subgraph_weight.shape) == (3,) and torch.isfinite(task.subgraph_weight).all()

"""CPU-side tests of the heterogeneous data layer and models (sgl_amd/hetero.py, sgl_amd/models/hetero, the base models): the
restatement of sample_by_edge_type against the reference's recorded sub-graphs, the properties of the seeded sub-graph draw, the
argument contract of the graph, the models and the task, and the `sgl.models.hetero` alias."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import ensemble_common as ec

from sgl_amd import hetero as het
from sgl_amd.models import hetero as models
from sgl_amd.models.base_model import BaseHeteroSGAPModel, FastBaseHeteroSGAPModel

REFERENCE_ROOT = "/root/reference"


def test_restated_sample_by_edge_type_equals_the_reference_bit_for_bit(goldens):
    g = goldens.npz("g23_hetero")
    args = ec.g23_graph_args(g)
    seen = 0
    for k, types_, undirected in ec.g23_samples(g):
        rowptr, col, val, x, node_id = ec.sample_by_edge_type_numpy(args, types_, undirected)
        for name, got in (("rowptr", rowptr), ("col", col), ("val", val), ("x", x), ("node_id", node_id)):
            want = g[f"sample|{k}|{name}"]
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (k, types_, name)
        seen += 1
    assert seen >= 6
    # the fixture holds what the issue asks for: a same-type edge type, one stored in both directions, repeats that count once
    a, b = "paper__to__author", "author__to__paper"
    assert np.array_equal(args["row_dict"][a], args["col_dict"][b]) and np.array_equal(args["col_dict"][a], args["row_dict"][b])
    rp = ec.sample_by_edge_type_numpy(args, ["paper__to__paper"])[0]
    assert rp[-1] < len(args["row_dict"]["paper__to__paper"])          # duplicates were merged, the same-type list is not mirrored


EDGE_TYPES = ["paper__to__author", "paper__to__paper", "paper__to__venue", "author__to__paper", "author__to__author", "author__to__venue",
              "venue__to__paper", "venue__to__author", "venue__to__venue", "paper__to__keyword", "keyword__to__paper", "keyword__to__keyword"]


def test_properties_of_the_seeded_subgraph_draw():
    unique = het._without_reverse_duplicates(EDGE_TYPES)
    assert unique == ["paper__to__author", "paper__to__paper", "paper__to__venue", "author__to__author", "author__to__venue",
                      "venue__to__venue", "paper__to__keyword", "keyword__to__keyword"]
    for predict, k, want in (("paper", 3, 6), ("venue", 2, 5), ("keyword", 4, 4)):
        for seed in (0, 1, 7):
            found = het.choose_multi_subgraphs(want, k, EDGE_TYPES, predict, seed)
            assert found == het.choose_multi_subgraphs(want, k, EDGE_TYPES, predict, seed)         # same seed, same draw
            assert len(found) == want and len(set(found)) == want                                    # distinct
            for combo in found:
                assert isinstance(combo, tuple) and list(combo) == sorted(combo) and len(set(combo)) == k
                assert set(combo) <= set(unique)                                                     # no reverse duplicate
                reached, left = {predict}, list(combo)                                               # grown from the predict class
                while left:
                    nxt = [e for e in left if set(e.split("__to__")) & reached]
                    assert nxt, (combo, predict)
                    for e in nxt:
                        reached |= set(e.split("__to__"))
                        left.remove(e)
        assert het.choose_multi_subgraphs(want, k, EDGE_TYPES, predict, 0) != het.choose_multi_subgraphs(want, k, EDGE_TYPES, predict, 5) or want == 1
    assert het.choose_multi_subgraphs(3, 9, EDGE_TYPES, "paper", 0) == []                            # more edge types than there are
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        few = het.choose_multi_subgraphs(50, 1, EDGE_TYPES, "keyword", 0)                            # only two single types touch it
    assert sorted(few) == [("keyword__to__keyword",), ("paper__to__keyword",)] and any("subgraphs" in str(x.message) for x in w)


def small_graph(**over):
    args = dict(row_dict={"a__to__b": [0, 1], "b__to__b": [3, 4]}, col_dict={"a__to__b": [3, 4], "b__to__b": [4, 5]},
                edge_weight_dict={"a__to__b": [1.0, 1.0], "b__to__b": [1.0, 1.0]}, num_node_dict={"a": 3, "b": 3}, node_types=["a", "b"],
                edge_types=["a__to__b", "b__to__b"], node_id_dict=None, x_dict={"a": np.ones((3, 2), np.float32), "b": np.zeros((3, 2), np.float32)},
                y_dict={"a": np.array([0, 1, 0])}, device="cpu")
    args.update(over)
    return het.HeteroGraph(**args)


def test_graph_and_dataset_contract():
    g = small_graph()
    assert g.node_types == ["a", "b"] and g.num_node == {"a": 3, "b": 3} and g.node_id_dict == {"a": [0, 1, 2], "b": [3, 4, 5]}
    assert g.num_features == {"a": 2, "b": 2} and g.num_classes == {"a": 2} and g["a__to__b"].num_edge == 2 and g["b"].num_node == 3
    small_graph(node_id_dict={"a": [0, 1, 2], "b": np.array([3, 4, 5])})                            # the default ids, spelled out
    for bad in ({"a": [0, 1, 2], "b": [5, 4, 3]}, {"a": [1, 2, 3], "b": [4, 5, 6]}, {"a": [0, 1], "b": [3, 4, 5]}):
        with pytest.raises(ValueError, match="contiguous"):
            small_graph(node_id_dict=bad)
    with pytest.raises(ValueError):
        small_graph(edge_types=["a__to__b"])
    with pytest.raises(TypeError):
        small_graph(node_types=("a", "b"))
    with pytest.raises(ValueError):
        g["c"]
    ds = het.HeteroNodeDataset(g, [0], [1], [2])
    assert ds.data is g and ds.node_types == g.node_types and ds.edge_types == g.edge_types and ds.train_idx == [0]
    with pytest.raises(TypeError):
        ds.sample_by_edge_type(3)
    with pytest.raises(TypeError):
        ds.sample_by_edge_type(["a__to__b", 3])
    with pytest.raises(TypeError):
        het.HeteroNodeDataset("not a graph")


def test_models_refuse_what_the_reference_refuses():
    ds = het.HeteroNodeDataset(small_graph())
    for cls in (models.NARS_SIGN, models.Fast_NARS_SGC_WithLearnableWeights):
        model = cls(2, 2, 2, 4, 2, 2)
        assert isinstance(model, (BaseHeteroSGAPModel, FastBaseHeteroSGAPModel))
        with pytest.raises(ValueError, match="Either subgraph_list or"):
            model.preprocess(ds, "a")
        with pytest.raises(ValueError, match="will be ignored"):
            model.preprocess(ds, "a", random_subgraph_num=2, subgraph_list=[])
        with pytest.raises(TypeError, match="HeteroNodeDataset"):
            model.preprocess("dataset", "a", subgraph_list=[])
        with pytest.raises(ValueError, match="valid node class"):
            model.preprocess(ds, "c", subgraph_list=[])
        with pytest.raises(ValueError, match="0 of the given sub-graphs touch 'a'.*random_subgraph_num=2"):
            model.preprocess(ds, "a", subgraph_list=[(("b__to__b",), None)])                         # skipped: does not touch 'a'
        with pytest.raises(TypeError, match="bfloat16"):
            cls(2, 2, 2, 4, 2, 2, hop_dtype="bfloat16")
    from sgl_amd.tricks import hetero_node_classification
    with pytest.raises(ValueError, match="Either subgraph_list or"):
        hetero_node_classification(models.NARS_SIGN(2, 2, 2, 4, 2, 2), ds, "a", 1, 0.01, 0.0)
    with pytest.raises(ValueError, match="will be ignored"):
        hetero_node_classification(models.NARS_SIGN(2, 2, 2, 4, 2, 2), ds, "a", 1, 0.01, 0.0, random_subgraph_num=2, subgraph_list=[])


def test_sgl_models_hetero_resolves_without_a_reference_checkout():
    from sgl_amd import compat
    assert not any(k == "sgl" or k.startswith("sgl.") for k in sys.modules)
    try:
        assert "sgl.models.hetero" in compat.install()
        from sgl.models.base_model import BaseHeteroSGAPModel as B1
        from sgl.models.hetero import NARS_SIGN, Fast_NARS_SGC_WithLearnableWeights
        from sgl.models.simple_models import FastOneDimConvolution, OneDimConvolution, OneDimConvolutionWeightSharedAcrossFeatures  # noqa: F401
        assert NARS_SIGN is models.NARS_SIGN and Fast_NARS_SGC_WithLearnableWeights is models.Fast_NARS_SGC_WithLearnableWeights
        assert B1 is BaseHeteroSGAPModel
    finally:
        compat.uninstall()
    assert not any(k == "sgl" or k.startswith("sgl.") for k in sys.modules)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE_ROOT, "sgl", "models", "hetero")),
                    reason="needs the reference checkout (build container only; nothing of it is copied or shipped)")
def test_reference_hetero_model_files_build_on_the_alias(goldens, monkeypatch):
    import inspect
    from sgl_amd import compat
    monkeypatch.setattr(sys, "dont_write_bytecode", True)            # the reference tree is read-only
    g = goldens.npz("g23_hetero")
    try:
        for name in ("NARS_SIGN", "Fast_NARS_SGC_WithLearnableWeights"):
            cls = compat.load_reference_model(name, REFERENCE_ROOT)
            assert inspect.getsourcefile(cls).startswith(REFERENCE_ROOT + "/sgl/models/hetero/"), name
            assert cls.__mro__[1].__module__ == "sgl_amd.models.base_model", name
            model = cls(*ec.G23_MODEL.values(), 3)
            assert type(model._aggregator).__module__ == "sgl_amd.models.simple_models"
            keys = [str(k) for k in g[f"model|{name}|keys"]]
            assert list(model.state_dict().keys()) == keys
            model.load_state_dict({k: torch.from_numpy(g[f"model|{name}|param|{k}"]) for k in keys})
    finally:
        compat.uninstall()
    assert not any(k == "sgl" or k.startswith("sgl.") for k in sys.modules)

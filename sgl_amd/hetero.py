"""Heterogeneous graphs on the device: the data the NARS models read (sgl/data/base_data.py HeteroGraph, sgl/data/base_dataset.py
HeteroNodeDataset, sgl/dataset/choose_edge_type.py), with the edge lists and the features resident on one GPU.

  HeteroGraph          the reference's constructor arguments; edge ends are GLOBAL node ids, the node types are contiguous id ranges
                       in `node_types` order (the only layout the reference's start_pos arithmetic supports: anything else raises).
  HeteroNodeDataset    a graph and the three index sets; sample_by_edge_type / nars_preprocess as in the reference, the relation
                       sub-graph built ON the device: local ids, the mirror of an edge type whose two ends differ in type, all lists
                       through io.coo_to_csr_device once, every stored value 1.0 (the reference's `adj.data = ones`).
  choose_multi_subgraphs   the reference's ChooseMultiSubgraphs under a seed.  The reference walks a Python set of strings, so its draw
                       depends on the interpreter's hash seed; here candidates are walked in list order and drawn from random.Random(seed):
                       the same properties (sorted tuples, distinct, connected to the predict class, reverse duplicates removed), the
                       same draw for the same seed.

Not here: sample_by_meta_path (a sparse x sparse product the reference itself calls extremely slow; neither model uses it)."""
import math
import random
import warnings

import numpy as np
import torch

from . import io

__all__ = ["HeteroGraph", "HeteroNodeDataset", "choose_multi_subgraphs", "edge_type_ends"]

EDGE_TYPE_DELIMITER = "__to__"


def edge_type_ends(edge_type):
    """('paper', 'author') of 'paper__to__author'"""
    parts = edge_type.split("__")
    if len(parts) != 3 or not parts[0] or not parts[2]:
        raise ValueError(f"an edge type reads '<source type>__<relation>__<target type>', not {edge_type!r}")
    return parts[0], parts[2]


def _check_edge_types(edge_types):
    if not isinstance(edge_types, (str, list, tuple)):
        raise TypeError("The given edge types must be a string or a list or a tuple!")
    if isinstance(edge_types, str):
        return [edge_types]
    for edge_type in edge_types:
        if not isinstance(edge_type, str):
            raise TypeError("Edge type must be a string!")
    return list(edge_types)


class _Node:
    def __init__(self, node_type, num_node, x, y, node_ids):
        self.node_type, self.num_node, self.x, self.y, self.node_ids = node_type, num_node, x, y, node_ids


class _Edge:
    def __init__(self, edge_type, row, col, edge_weight):
        self.edge_type, self.edge_index, self.edge_weight, self.num_edge = edge_type, (row, col), edge_weight, int(row.numel())


class HeteroGraph:
    def __init__(self, row_dict, col_dict, edge_weight_dict, num_node_dict, node_types, edge_types, node_id_dict=None,
                 x_dict=None, y_dict=None, edge_attr_dict=None, device="cuda"):
        if not isinstance(node_types, list) or not isinstance(edge_types, list):
            raise TypeError("Node types and edge types must be lists!")
        if any(not isinstance(t, str) for t in node_types + edge_types):
            raise TypeError("Node types and edge types must be strings!")
        if not isinstance(num_node_dict, dict) or sorted(num_node_dict) != sorted(node_types):
            raise TypeError("The keys of num_nodes and node_types must be the same!")
        if any(v is not None and not isinstance(v, dict) for v in (x_dict, y_dict, edge_attr_dict)):
            raise TypeError("Xs, Ys and edge attrs must be dicts!")
        if not all(isinstance(v, dict) for v in (row_dict, col_dict, edge_weight_dict)):
            raise TypeError("Rows, cols and edge weights must be dicts!")
        if not (sorted(row_dict) == sorted(col_dict) == sorted(edge_weight_dict) == sorted(edge_types)):
            raise ValueError("The keys of the rows, cols, edge_weights and edge_types must be the same!")
        self.device = torch.device(device)
        self.__node_types, self.__edge_types = node_types, edge_types
        self.__offsets, count = {}, 0
        for t in node_types:
            self.__offsets[t] = count
            count += int(num_node_dict[t])
        self.__total = count
        self.__node_id_dict = {t: list(range(self.__offsets[t], self.__offsets[t] + int(num_node_dict[t]))) for t in node_types}
        if node_id_dict is not None:
            for t in node_types:
                given = np.asarray(node_id_dict[t]).reshape(-1)
                if given.shape[0] != len(self.__node_id_dict[t]) or not np.array_equal(given, self.__node_id_dict[t]):
                    raise ValueError(f"node ids of {t!r} are not the contiguous default range [{self.__offsets[t]}, "
                                     f"{self.__offsets[t] + int(num_node_dict[t])}): only that layout is supported")
        x_dict, y_dict = x_dict or {}, y_dict or {}
        self.__nodes = {}
        for t in node_types:
            x = x_dict.get(t)
            if x is not None:
                x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(device=self.device, dtype=torch.float32).contiguous()
                if x.dim() != 2 or x.shape[0] != int(num_node_dict[t]):
                    raise ValueError(f"features of {t!r} must be [{int(num_node_dict[t])}, d]")
            self.__nodes[t] = _Node(t, int(num_node_dict[t]), x, y_dict.get(t), self.__node_id_dict[t])
        self.__edges = {}
        for e in edge_types:
            edge_type_ends(e)
            row = torch.as_tensor(row_dict[e]).to(device=self.device, dtype=torch.int64).contiguous().view(-1)
            col = torch.as_tensor(col_dict[e]).to(device=self.device, dtype=torch.int64).contiguous().view(-1)
            if row.numel() != col.numel():
                raise ValueError(f"row and col of {e!r} differ in length")
            self.__edges[e] = _Edge(e, row, col, edge_weight_dict[e])
        self.edge_attr_dict = edge_attr_dict

    def __getitem__(self, key):
        if key in self.__edges:
            return self.__edges[key]
        if key in self.__nodes:
            return self.__nodes[key]
        raise ValueError("Please input valid edge type or node type!")

    node_id_dict = property(lambda self: self.__node_id_dict)
    nodes = property(lambda self: self.__nodes)
    edges = property(lambda self: self.__edges)
    node_types = property(lambda self: self.__node_types)
    edge_types = property(lambda self: self.__edge_types)
    node_id_offsets = property(lambda self: dict(self.__offsets))
    num_node = property(lambda self: {t: self.__nodes[t].num_node for t in self.__node_types})
    num_features = property(lambda self: {t: 0 if self.__nodes[t].x is None else int(self.__nodes[t].x.shape[1]) for t in self.__node_types})

    @property
    def num_classes(self):
        return {t: int(np.asarray(self.__nodes[t].y).max()) + 1 for t in self.__node_types if self.__nodes[t].y is not None}


# ---- the sub-graph draw (sgl/dataset/choose_edge_type.py) ------------------------------------------------------------------------------
def _without_reverse_duplicates(edge_types):
    kept = []
    for et in edge_types:
        a, b = et.split(EDGE_TYPE_DELIMITER)
        if b + EDGE_TYPE_DELIMITER + a not in kept:
            kept.append(et)
    return kept


def _choose_edge_types(edge_type_num, edge_types, predict_class, rng):
    explored, chosen, candidates, others = {predict_class}, [], [], list(edge_types)
    for _ in range(edge_type_num):
        reach = [et for et in others if set(et.split(EDGE_TYPE_DELIMITER)) & explored]
        candidates += reach
        others = [et for et in others if et not in reach]
        if not candidates:
            warnings.warn(f"Can't find enough ({edge_type_num}) edge types!", UserWarning)
            break
        pick = rng.choice(candidates)
        chosen.append(pick)
        candidates.remove(pick)
        explored |= set(pick.split(EDGE_TYPE_DELIMITER))
    return tuple(sorted(chosen))


def choose_multi_subgraphs(subgraph_num, edge_type_num, edge_types, predict_class, seed=0):
    """up to subgraph_num distinct sorted tuples of edge_type_num edge types, each grown from predict_class along shared node types"""
    rng = random.Random(seed)
    unique = _without_reverse_duplicates(list(edge_types))
    found = []
    if edge_type_num > len(unique):
        return found
    ways = math.comb(len(unique), edge_type_num)
    budget, steps = 10 * ways * (math.log2(ways) + 1), 0
    for _ in range(subgraph_num):
        while True:
            steps += 1
            if steps > budget:                                   # (coupon collector: enough draws to have seen every combination)
                warnings.warn(f"Can't find enough ({subgraph_num}) subgraphs!", UserWarning)
                break
            combo = _choose_edge_types(edge_type_num, unique, predict_class, rng)
            if combo in found:
                continue
            if combo:
                found.append(combo)
            break
    return found


class HeteroNodeDataset:
    def __init__(self, data, train_idx=None, val_idx=None, test_idx=None, name="hetero"):
        if not isinstance(data, HeteroGraph):
            raise TypeError("data must be a HeteroGraph")
        self._data, self._name = data, name
        self._train_idx, self._val_idx, self._test_idx = train_idx, val_idx, test_idx

    data = property(lambda self: self._data)
    name = property(lambda self: self._name)
    node_types = property(lambda self: self._data.node_types)
    edge_types = property(lambda self: self._data.edge_types)
    train_idx = property(lambda self: self._train_idx)
    val_idx = property(lambda self: self._val_idx)
    test_idx = property(lambda self: self._test_idx)

    def sample_by_edge_type(self, edge_types, undirected=True):
        """(DeviceAdjacency, X, node_id) of the relation sub-graph over the node types the given edge types touch"""
        edge_types = _check_edge_types(edge_types)
        data = self._data
        touched = {t for e in edge_types for t in edge_type_ends(e)}
        offsets, local = data.node_id_offsets, {}
        num_node, feats, node_id = 0, [], []
        for t in data.node_types:                               # the sampled types keep the graph's order
            if t not in touched:
                continue
            local[t] = offsets[t] - num_node                    # global id - local[t] = id inside the sub-graph
            num_node += data.num_node[t]
            if data[t].x is None:
                raise ValueError(f"{t} nodes have no features!")
            feats.append(data[t].x)
            node_id += data.node_id_dict[t]
        if len({f.shape[1] for f in feats}) != 1:
            raise ValueError("the sampled node types have features of different widths")
        rows, cols = [], []
        for e in edge_types:
            src, dst = edge_type_ends(e)
            row, col = data[e].edge_index
            row, col = row - local[src], col - local[dst]
            if undirected is True and src != dst:
                row, col = torch.cat((row, col)), torch.cat((col, row))
            rows.append(row)
            cols.append(col)
        rows, cols = torch.cat(rows), torch.cat(cols)
        adj = io.coo_to_csr_device(rows, cols, torch.ones(rows.numel(), dtype=torch.float32, device=data.device), num_node, device=data.device)
        adj.val.fill_(1.0)                                      # edges given more than once count once
        x = feats[0] if len(feats) == 1 else torch.cat(feats, dim=0)
        return adj, x, torch.LongTensor(node_id)

    def nars_preprocess(self, edge_types, predict_class, random_subgraph_num, subgraph_edge_type_num, seed=0):
        """{edge type tuple: sample_by_edge_type(tuple)} for random_subgraph_num of the combinations choose_multi_subgraphs finds"""
        edge_types = _check_edge_types(edge_types)
        combos = choose_multi_subgraphs(random_subgraph_num, subgraph_edge_type_num, edge_types, predict_class, seed)
        if random_subgraph_num > len(combos):
            random_subgraph_num = len(combos)
            warnings.warn("The input random_subgraph_num exceeds the number of all the combinations of edge types!"
                          f"\nThe random_subgraph_num has been set to {len(combos)}.", UserWarning)
        order = np.random.default_rng(seed).permutation(len(combos))[:random_subgraph_num]
        return {combos[i]: self.sample_by_edge_type(combos[i]) for i in order}

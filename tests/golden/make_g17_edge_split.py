#!/usr/bin/env python3
"""Generate tests/golden/g17_edge_split.npz by IMPORTING THE REFERENCE ITSELF (as make_g14_link_prediction.py does).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g17_edge_split.py <path of the reference checkout>

Needs the reference checkout (the directory that holds its `sgl` package) and sklearn (which its sgl/tasks/utils.py imports); nothing of the reference
travels: the fixture holds recorded outputs only.

G17: mask_test_edges (sgl/tasks/utils.py:148-259) on the graphs sym64, pl256 and dir40 of graphs.npz under np.random.seed(17): the
seven values it returns -- adj_train as CSR arrays, the six edge lists as int64 [*, 2].  The tests do not compare our split with
these draws (the reference's come from numpy's global generator); they pin tests/edge_split_common.check_split to what the reference
really returns, and the sizes of the seven outputs."""
import importlib
import os
import sys
import types
from unittest.mock import MagicMock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np
import scipy.sparse as sp

GRAPHS = ("sym64", "pl256", "dir40")
SEED = 17
NAMES = ("train_edges", "train_edges_false", "val_edges", "val_edges_false", "test_edges", "test_edges_false")


def graph(name):
    g = np.load(os.path.join(HERE, "graphs.npz"))
    indptr, indices, data = g[name + "|indptr"], g[name + "|indices"], g[name + "|data"]
    n = len(indptr) - 1
    return sp.csr_matrix((data, indices, indptr), shape=(n, n))


def reference_utils_module():
    for m in ["matplotlib", "matplotlib.pyplot", "munkres"]:
        try:
            importlib.import_module(m)
        except ImportError:
            sys.modules[m] = MagicMock()
    if "sgl.tasks" not in sys.modules:
        pkg = types.ModuleType("sgl.tasks")
        pkg.__path__ = [REF + "/sgl/tasks"]
        sys.modules["sgl.tasks"] = pkg
    import sgl.tasks.utils as utils
    return utils


def main():
    utils = reference_utils_module()
    out = {"seed": np.array(SEED), "graphs": np.array(GRAPHS)}
    for name in GRAPHS:
        np.random.seed(SEED)
        got = utils.mask_test_edges(graph(name))
        adj_train = sp.csr_matrix(got[0])
        adj_train.sum_duplicates()
        adj_train.sort_indices()
        out[f"{name}|adj_train|indptr"] = adj_train.indptr.astype(np.int64)
        out[f"{name}|adj_train|indices"] = adj_train.indices.astype(np.int32)
        out[f"{name}|adj_train|data"] = adj_train.data.astype(np.float32)
        for key, t in zip(NAMES, got[1:]):
            out[f"{name}|{key}"] = t.numpy().astype(np.int64).reshape(-1, 2)
        print(name, {key: tuple(out[f"{name}|{key}"].shape) for key in NAMES})
    np.savez_compressed(os.path.join(HERE, "g17_edge_split.npz"), **out)


if __name__ == "__main__":
    main()

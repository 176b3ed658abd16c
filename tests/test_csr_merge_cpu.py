"""CPU-side checks of the CSR merge (csrc/sgl_csr_merge.hip, device.csr_merge, sgl_amd/transforms.py add_edges / add_self_loops /
to_undirected): the two exported symbols and their bindings, their refusals without a GPU -- a non-zero code and a message that names
the entry, nothing launched -- the tests' numpy reference against a plain two-pointer loop, against scipy's csr_matrix of the
concatenated lists and against what the REFERENCE's transforms returned (tests/golden/g22_merge_transforms.npz), two wrong slot
rules that the zoo must be able to see, and the argument checks of the Python layer."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT

import csr_merge_common as common
from sgl_amd import _lib

ROWPTR, FILL = "sgl_csr_merge_rowptr", "sgl_csr_merge_fill"
ZOO = common.shared_zoo()


@pytest.mark.parametrize("name", [ROWPTR, FILL])
def test_library_exports_the_symbols(name):
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, name), f"{name} is not exported by libsgl_hip.so"
    assert name in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 110


@pytest.mark.parametrize("name,count", [(ROWPTR, 12), (FILL, 18)])
def test_header_and_binding_argument_counts_agree(name, count):
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    assert name in text[:text.index("#ifndef SGL_HIP_H")], "the symbol list at the top of the header"
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sgl_hip.h"
    params = [p for p in m.group(1).split(",") if p.strip()]
    restype, argtypes = _lib.PROTOTYPES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == count, (len(argtypes), params)
    for word in ("a_rowptr", "a_col", "nnz_a", "b_rowptr", "b_col", "nnz_b", "n_rows", "n_cols", "lanes", "d_out_rowptr"):
        assert word in m.group(1), word
    assert re.search(r"#define\s+SGL_MERGE_SUM\s+0\b", text) and re.search(r"#define\s+SGL_MERGE_KEEP_A\s+1\b", text)
    assert (_lib.SGL_MERGE_SUM, _lib.SGL_MERGE_KEEP_A) == (common.SUM, common.KEEP) == (0, 1)


def test_public_names_are_exported():
    import sgl_amd
    from sgl_amd import device as dev
    from sgl_amd import transforms as tr
    for name in ("add_edges", "add_self_loops", "to_undirected"):
        assert name in tr.__all__ and callable(getattr(tr, name))
    for name in ("get_subgraph", "drop_edges", "remove_self_loops", "mask_features"):     # the existing ones are still there
        assert name in tr.__all__
    assert not hasattr(tr, "delete_repeated_edges") and not hasattr(tr, "sort_edges")     # canonical by construction: not ported
    assert sgl_amd.transforms is tr
    assert callable(dev.csr_merge) and dev.CSR_MERGE_LANES == common.LANES
    assert dev.CSR_MERGE_MODES == common.MODES


class Args:
    """calls on HOST memory that is never touched: every bad call is refused before anything is launched.  A 4 x 4 pair."""

    def __init__(self):
        self.buf = {k: (ctypes.c_int64 * 16)() for k in ("a_rowptr", "a_col", "a_val", "b_rowptr", "b_col", "b_val", "out_rowptr", "out_col",
                                                          "out_val", "out_pos_a", "out_pos_b")}
        p = {k: ctypes.cast(v, ctypes.c_void_p) for k, v in self.buf.items()}
        self.nnz_out = ctypes.c_int64(-7)
        self.base = dict(p, nnz_a=6, nnz_b=5, n_rows=4, n_cols=4, mode=0, lanes=0)

    @staticmethod
    def off(p, k):
        return ctypes.c_void_p(p.value + k)

    def call_rowptr(self, **change):
        k = dict(self.base, **change)
        return _lib.lib().sgl_csr_merge_rowptr(k["a_rowptr"], k["a_col"], k["nnz_a"], k["b_rowptr"], k["b_col"], k["nnz_b"], k["n_rows"], k["n_cols"],
                                               k["lanes"], k["out_rowptr"], ctypes.byref(self.nnz_out), None)

    def call_fill(self, **change):
        k = dict(self.base, **change)
        return _lib.lib().sgl_csr_merge_fill(k["a_rowptr"], k["a_col"], k["a_val"], k["nnz_a"], k["b_rowptr"], k["b_col"], k["b_val"], k["nnz_b"],
                                             k["n_rows"], k["n_cols"], k["mode"], k["lanes"], k["out_rowptr"], k["out_col"], k["out_val"],
                                             k["out_pos_a"], k["out_pos_b"], None)


def refused(call, name, **change):
    rc = call(**change)
    msg = _lib.last_error()
    assert rc != 0, change
    assert msg and name in msg, (change, msg)


@pytest.mark.parametrize("which", [ROWPTR, FILL])
def test_bad_arguments_are_refused_without_a_gpu(which):
    a = Args()
    call = a.call_rowptr if which == ROWPTR else a.call_fill
    b = a.base
    for key in ("n_rows", "n_cols", "nnz_a", "nnz_b"):
        refused(call, which, **{key: -1})
    refused(call, which, n_rows=1 << 31)
    refused(call, which, n_cols=1 << 31)
    for key in ("a_rowptr", "a_col", "b_rowptr", "b_col"):
        refused(call, which, **{key: None})
    for lanes in (-1, 1, 2, 8, 32, 63, 65, 128):
        refused(call, which, lanes=lanes)
    refused(call, which, a_rowptr=a.off(b["a_rowptr"], 4))
    refused(call, which, b_rowptr=a.off(b["b_rowptr"], 4))
    refused(call, which, a_col=a.off(b["a_col"], 2))
    refused(call, which, b_col=a.off(b["b_col"], 1))
    if which == ROWPTR:
        refused(call, which, out_rowptr=None)
        refused(call, which, out_rowptr=a.off(b["out_rowptr"], 4))
        assert a.nnz_out.value == -7                          # never written by a refused call
    else:
        for mode in (-1, 2, 3):
            refused(call, which, mode=mode)
        for key in ("a_val", "b_val", "out_rowptr", "out_col", "out_val"):
            refused(call, which, **{key: None})
        refused(call, which, a_val=a.off(b["a_val"], 2))
        refused(call, which, b_val=a.off(b["b_val"], 2))
        refused(call, which, out_rowptr=a.off(b["out_rowptr"], 4))
        refused(call, which, out_col=a.off(b["out_col"], 2))
        refused(call, which, out_val=a.off(b["out_val"], 2))
        refused(call, which, out_pos_a=a.off(b["out_pos_a"], 4))
        refused(call, which, out_pos_b=a.off(b["out_pos_b"], 4))
        assert a.call_fill(nnz_a=0, nnz_b=0) == 0, _lib.last_error()        # nothing to write: no launch, no device needed
        assert a.call_fill(n_rows=0, out_pos_a=None, out_pos_b=None, mode=1) == 0, _lib.last_error()


def test_the_lanes_rule_is_k13s_on_the_longer_side():
    text = open(os.path.join(ROOT, "sgl_amd", "csrc", "sgl_csr_merge.hip")).read()
    assert "std::max(nnz_a, nnz_b) / n_rows" in text and "mean < 8 ? 4 : mean < 32 ? 16 : 64" in text
    select = open(os.path.join(ROOT, "sgl_amd", "csrc", "sgl_csr_select.hip")).read()
    assert "mean < 8 ? 4 : mean < 32 ? 16 : 64" in select
    for g in common.LANES:
        assert f"csr_merge_kernel<{g}, FILL>" in text


# ---- the numpy reference ------------------------------------------------------------------------------------------------------------
def test_the_zoo_holds_what_it_promises():
    a, b = ZOO["main"]
    assert a.shape == b.shape == (261, 7001) and max(m.shape[0] for pair in ZOO.values() for m in pair) <= 300
    la, lb = np.diff(a.indptr), np.diff(b.indptr)
    pairs = set(zip(la.tolist(), lb.tolist()))
    for x in common.ZOO_LENGTHS:
        for y in common.ZOO_LENGTHS:
            assert (x, y) in pairs
    assert {(0, 0), (0, 3), (3, 0), (3001, 1), (1, 3001), (3000, 3000)} <= pairs
    assert la[0] == lb[0] == la[-1] == lb[-1] == 0
    want = common.merge_reference(a, b)
    both = (want[3] >= 0) & (want[4] >= 0)
    for pos, ptr in ((want[3], a.indptr), (want[4], b.indptr)):            # common columns on both sides of every stride boundary
        rank = pos[both] - ptr[np.searchsorted(ptr, pos[both], side="right") - 1]
        assert set(common.BOUNDARIES) <= set(rank.tolist())
    bits = set(np.concatenate((a.data, b.data)).view(np.uint32).tolist())
    assert set(common.SPECIAL_A.tolist()) | set(common.SPECIAL_B.tolist()) <= bits
    out = set(want[2].view(np.uint32).tolist())
    assert {0x7FC01234, 0xFFC0ABCD, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x00000002} <= out
    sq = common.merge_reference(*ZOO["square"])
    assert ((sq[3] >= 0) & (sq[4] >= 0) & (sq[2] == 0)).sum() >= 10         # cancelled pairs stay as stored zeros
    assert ZOO["a_empty"][0].nnz == 0 and ZOO["b_empty"][1].nnz == 0 and ZOO["both_empty"][0].nnz == ZOO["both_empty"][1].nnz == 0
    assert ZOO["one_row"][0].shape[0] == 1 and ZOO["tall"][0].shape == (203, 11)


@pytest.mark.parametrize("case", sorted(ZOO))
def test_reference_equals_the_two_pointer_loop(case):
    a, b = ZOO[case]
    for mode in (common.SUM, common.KEEP):
        assert common.agrees(common.merge_reference(a, b, mode), common.merge_loop(a, b, mode)), mode


@pytest.mark.parametrize("case", sorted(ZOO))
def test_reference_sum_equals_scipy_of_the_concatenated_lists(case):
    """bit for bit: every pair occurs at most twice in the concatenation, and one float32 addition commutes"""
    a, b = ZOO[case]
    want = common.scipy_concatenated(a, b)
    got = common.merge_reference(a, b, common.SUM)
    assert np.array_equal(got[0], want.indptr) and np.array_equal(got[1], want.indices) and common.same_bits(got[2], want.data.astype(np.float32))
    keep = common.merge_reference(a, b, common.KEEP)
    assert np.array_equal(keep[0], got[0]) and np.array_equal(keep[1], got[1])
    both = (keep[3] >= 0) & (keep[4] >= 0)
    assert common.same_bits(keep[2][keep[3] >= 0], a.data[keep[3][keep[3] >= 0]].astype(np.float32))       # every stored value of A, untouched
    assert common.same_bits(keep[2][~both & (keep[4] >= 0)], b.data[keep[4][~both & (keep[4] >= 0)]].astype(np.float32))


@pytest.mark.parametrize("case", sorted(ZOO))
def test_the_slot_rule_and_two_wrong_ones(case):
    a, b = ZOO[case]
    want = common.merge_reference(a, b)
    right = common.slot_fill(a, b, want[0], "right")
    assert np.array_equal(right[0], want[1]) and np.array_equal(right[1], want[3]) and np.array_equal(right[2], want[4])
    seen = common.common_followed(a, b)
    assert seen == (case in ("main", "one_row", "square", "tall"))
    for rule in ("no_common", "upper"):
        wrong = common.slot_fill(a, b, want[0], rule)
        differs = not (np.array_equal(wrong[0], want[1]) and np.array_equal(wrong[1], want[3]) and np.array_equal(wrong[2], want[4]))
        assert differs == seen, rule


def test_wrong_rules_show_in_every_row_with_a_followed_common_column():
    a, b = ZOO["main"]
    want = common.merge_reference(a, b)
    for rule in ("no_common", "upper"):
        wrong = common.slot_fill(a, b, want[0], rule)
        for i in range(a.shape[0]):
            s, e = want[0][i], want[0][i + 1]
            both = (want[3][s:e] >= 0) & (want[4][s:e] >= 0)
            followed = bool(both[:-1].any()) if e > s else False
            changed = not (np.array_equal(wrong[0][s:e], want[1][s:e]) and np.array_equal(wrong[1][s:e], want[3][s:e]))
            assert changed or not followed, (rule, i)


# ---- against the reference's recorded results -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", common.G22_GRAPHS)
def test_reference_model_against_g22(goldens, name):
    g = goldens.npz("g22_merge_transforms")
    a = common.g22_graph(goldens, name)
    n = a.shape[0]
    idx, w = g[f"{name}|add_idx"], g[f"{name}|add_w"]
    assert idx.shape == (2, 39) and w.dtype == np.float32
    added = common.storage_order_csr(idx, w, a.shape)
    got = common.as_matrix(common.merge_reference(a, added, common.SUM), a.shape)
    golden = common.recorded(goldens, f"{name}|add")
    common.check_against_add_golden(got, a, idx, w, golden)
    key, count = common.multiplicity(a, idx)
    triple = g[f"{name}|triple"]
    assert key[count == 3][0] == triple[0] * n + triple[1]
    assert ((golden.data == 0) & (count == 2)).sum() >= 1                                  # the cancelled pair: a stored zero
    got = common.as_matrix(common.merge_reference(a, added, common.KEEP), a.shape)
    common.check_against_del_golden(got, a, idx, w, common.recorded(goldens, f"{name}|add_del"))
    for key_, lw in (("loops", np.ones(n, dtype=np.float32)), ("loops_w", g[f"{name}|loop_w"])):
        eye = sp.csr_matrix((lw, np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, n))
        got = common.merge_reference(a, eye, common.SUM)
        want = common.recorded(goldens, f"{name}|{key_}")
        assert np.array_equal(got[0], want.indptr) and np.array_equal(got[1], want.indices) and common.same_bits(got[2], want.data)
        assert len(got[1]) == a.nnz + n - np.count_nonzero(common.keys(a) % (n + 1) == 0)
    lw = g[f"{name}|loop_w"]
    assert (lw == 0).sum() == 1 and (lw < 0).sum() == 1
    t = common.canonical(a.T.tocsr())
    got = common.merge_reference(a, t, common.SUM)
    want = common.recorded(goldens, f"{name}|und")
    assert np.array_equal(got[0], want.indptr) and np.array_equal(got[1], want.indices) and common.same_bits(got[2], want.data)
    m = common.as_matrix(got, a.shape)
    assert (abs(m - m.T) > 0).nnz == 0
    if name == "dir40":
        assert len(got[1]) > a.nnz                                                         # the directed graph gains the missing directions
    if name == "symdiag48":
        assert np.array_equal(m.diagonal(), 2 * a.diagonal()) and np.count_nonzero(a.diagonal()) > 10       # the doubled diagonal


# ---- the Python layer's argument checks (no device is reached) ----------------------------------------------------------------------
def host_adjacency(a):
    from sgl_amd.io import DeviceAdjacency
    return DeviceAdjacency(torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int32)),
                           torch.from_numpy(a.data.astype(np.float32)), a.shape)     # a container of CPU tensors: refused before any launch


def test_error_messages_of_the_transforms_are_the_references(goldens):
    from sgl_amd import transforms as tr
    host = host_adjacency(common.g22_graph(goldens, "sym64"))
    for bad in (torch.zeros(3, 4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), np.zeros((2, 3, 1), dtype=np.int64), [1, 2, 3],
                [[0, 1], [1, 2], [2, 3]]):
        with pytest.raises(ValueError, match=re.escape("add indices must be in shape of (2, x)!")):
            tr.add_edges(host, bad)
    for bad in ([[0, 64], [1, 2]], [[0, 1], [64, 2]], torch.tensor([[0, -1], [1, 2]]), np.array([[0, 1], [-3, 2]]), [[1 << 40], [0]]):
        with pytest.raises(ValueError, match=re.escape("indices must be in range of [0, num_node)!")):
            tr.add_edges(host, bad)
        with pytest.raises(ValueError, match=re.escape("indices must be in range of [0, num_node)!")):
            tr.add_edges(host, bad, del_repeated=True)
    assert tr.add_edges(host, torch.zeros(2, 0, dtype=torch.int64)) is host            # an empty list: the input object
    assert tr.add_edges(host, [[], []], del_repeated=True) is host
    assert tr.add_edges(host, np.zeros((2, 0), dtype=np.int32), add_weights=np.zeros(0, dtype=np.float32)) is host
    for bad in (torch.ones(63), torch.ones(65), np.ones((64, 1), dtype=np.float32), np.zeros(0, dtype=np.float32), [1.0] * 3):
        with pytest.raises(ValueError, match=re.escape("add weights must be in shape of [num_node]!")):
            tr.add_self_loops(host, bad)
    from sgl_amd.io import DeviceAdjacency
    rect = DeviceAdjacency(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float32), (3, 5))
    with pytest.raises(ValueError, match="square"):
        tr.add_self_loops(rect)
    with pytest.raises(ValueError, match="square"):
        tr.to_undirected(rect)
    with pytest.raises(ValueError, match="reduce"):
        tr.to_undirected(host, reduce="max")


def test_loader_option_is_checked_before_anything_is_read(tmp_path):
    from sgl_amd import io
    import inspect
    assert inspect.signature(io.load_custom_homo_raw).parameters["undirected"].default is None
    with pytest.raises(ValueError, match="undirected"):
        io.load_custom_homo_raw(str(tmp_path), num_node=3, undirected="max")

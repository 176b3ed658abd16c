"""COO -> canonical CSR on a real MI355X (csrc/sgl_ingest.hip through io.coo_to_csr_device, io.load_custom_homo_raw_sharded and
reorder.permute_csr): run with `-m gpu`.

Row pointer, columns and the number of entries are integers; every value is one sequential float32 sum in storage order.  So every
comparison with the numpy reference of ingest_common is bit-exact, over a zoo whose weights make the order of a sum show in its bits
(tests/test_ingest_cpu.py holds the conditions), and scipy's bits are required wherever a pair is stored at most twice."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ingest_common as common
from sgl_amd import _lib, io, reorder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def build(cuda, z, row=None, col=None, val=None):
    """(rowptr, col, val, nnz) of the device build as numpy arrays"""
    row, col, val = (z[k] if a is None else a for k, a in (("row", row), ("col", col), ("val", val)))
    adj = io.coo_to_csr_device(row, col, val, z["n_rows"], device=cuda, num_col=z["n_cols"])
    assert adj.shape == (z["n_rows"], z["n_cols"]) and adj.rowptr.dtype == torch.int64 and adj.col.dtype == torch.int32
    assert adj.val.dtype == torch.float32 and adj.col.numel() == adj.val.numel()
    return adj.rowptr.cpu().numpy(), adj.col.cpu().numpy(), adj.val.cpu().numpy(), adj.nnz


def is_reference(got, want, what=""):
    rowptr, col, val, nnz = got
    assert np.array_equal(rowptr, want[0]) and rowptr.dtype == np.int64, what
    assert np.array_equal(col, want[1]) and col.dtype == np.int32, what
    assert nnz == want[3] == len(val), what
    nan = np.isnan(want[2])
    assert np.isnan(val[nan]).all(), what                                   # a NaN is a NaN, whatever its payload
    assert np.array_equal(common.bits(val[~nan]), common.bits(want[2][~nan])), what


@pytest.mark.parametrize("name", common.ZOO_NAMES)
def test_zoo_case_is_the_reference_bit_for_bit(cuda, name):
    z = common.BY_NAME[name]
    want = common.reference(name)
    lengths = want[4]
    on_device = [torch.from_numpy(z[k]).to(cuda) for k in ("row", "col", "val")]
    got = build(cuda, z, *on_device)
    is_reference(got, want, "device tensors")
    short = lengths <= 2
    assert common.same_values(got[2][short], np.asarray(common.scipy_csr(z).data, dtype=np.float32)[short])     # scipy's bits on runs <= 2
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        again = build(cuda, z, *on_device)
    side.synchronize()
    is_reference(again, want, "side stream")
    is_reference(build(cuda, z, z["row"].astype(np.int32), z["col"].astype(np.int32), z["val"]), want, "int32 numpy arrays")
    for t, k in zip(on_device, ("row", "col", "val")):                        # the inputs are only read
        assert np.array_equal(t.cpu().numpy().view(np.uint8), z[k].view(np.uint8)), k


@pytest.mark.parametrize("what,which,value", common.bad_indices(40, 50), ids=[b[0] for b in common.bad_indices(40, 50)])
def test_one_index_outside_is_an_error_and_the_next_call_is_right(cuda, what, which, value):
    """make_keys_kernel writes keys[i] and iota[i] only and the entry returns before anything is folded: nothing is read or written
    through the bad index"""
    z = common.error_list()
    assert (z["n_rows"], z["n_cols"]) == (40, 50) and len(z["row"]) == 600
    want = common.coo_to_csr_reference(z["row"], z["col"], z["val"], 40, 50)
    for at in (0, 255, 599):
        bad = {k: z[k].copy() for k in ("row", "col")}
        bad[which][at] = value
        with pytest.raises(_lib.SglHipError, match="outside"):
            build(cuda, z, torch.from_numpy(bad["row"]).to(cuda), torch.from_numpy(bad["col"]).to(cuda))
        is_reference(build(cuda, z), want, (what, at))


def test_mismatched_lengths_are_a_value_error(cuda):
    z = common.error_list()
    for cut in ("row", "col", "val"):
        arrays = {k: (z[k][:-1] if k == cut else z[k]) for k in ("row", "col", "val")}
        with pytest.raises(ValueError, match="same length"):
            io.coo_to_csr_device(arrays["row"], arrays["col"], arrays["val"], 40, device=cuda, num_col=50)


def stitched(parts):
    rowptr, col, val, at = [np.zeros(1, np.int64)], [], [], 0
    for q in parts:
        blk = q["block"]
        local = blk.rowptr.cpu().numpy()
        assert local[0] == 0 and local[-1] == blk.col.numel() == blk.val.numel()
        rowptr.append(local[1:] + at)
        at += int(local[-1])
        col.append(blk.col.cpu().numpy())
        val.append(blk.val.cpu().numpy())
    return np.concatenate(rowptr), np.concatenate(col), np.concatenate(val)


@pytest.mark.parametrize("world", [1, 3, 5])
def test_sharded_ingest_sums_in_storage_order_across_chunks(cuda, tmp_path, world):
    z = common.BY_NAME["sharded_square"]
    n, m = z["n_rows"], len(z["row"])
    want = common.reference("sharded_square")
    order, starts, lengths = common.sorted_runs(z["row"], z["col"], n)
    spread = [np.unique(order[s:s + k] // 97).size for s, k in zip(starts, lengths) if k >= 3]
    assert spread and min(spread) >= 2                                      # every run of three or more has members in different chunks of 97
    io.save_custom_homo_raw(str(tmp_path), z["row"], z["col"], z["val"])
    empty = 0
    for chunk in (1, 97, m + 1000):
        parts = [io.load_custom_homo_raw_sharded(str(tmp_path), r, world, num_node=n, device=cuda, chunk_edges=chunk) for r in range(world)]
        b = parts[0]["bounds"]
        assert b[0] == 0 and b[-1] == n and all(np.array_equal(b, q["bounds"]) for q in parts)
        for r, q in enumerate(parts):
            blk = q["block"]
            assert (blk.lo, blk.hi, blk.n) == (int(b[r]), int(b[r + 1]), n) and blk.rowptr.numel() == blk.hi - blk.lo + 1
            empty += blk.hi == blk.lo
        rowptr, col, val = stitched(parts)
        assert np.array_equal(rowptr, want[0]) and np.array_equal(col, want[1]) and col.dtype == np.int32, chunk
        assert np.array_equal(common.bits(val), common.bits(want[2])), chunk
    assert (empty > 0) == (world > 1)                                         # the heavy row leaves ranks without rows


def test_sharded_ingest_refuses_a_column_outside_in_the_last_chunk(cuda, tmp_path):
    z = common.BY_NAME["sharded_square"]
    n = z["n_rows"]
    col = z["col"].copy()
    col[-1] = n
    io.save_custom_homo_raw(str(tmp_path), z["row"], col, z["val"])
    with pytest.raises(_lib.SglHipError, match="outside"):
        io.load_custom_homo_raw_sharded(str(tmp_path), 0, 1, num_node=n, device=cuda, chunk_edges=97)
    owner = None
    for r in range(3):                                                      # the rank that owns the entry's row refuses; the others never see it
        try:
            q = io.load_custom_homo_raw_sharded(str(tmp_path), r, 3, num_node=n, device=cuda, chunk_edges=97)
            assert not (q["block"].lo <= z["row"][-1] < q["block"].hi)
        except _lib.SglHipError as e:
            assert "outside" in str(e) and owner is None
            owner = r
    assert owner is not None


def test_permute_csr_of_an_unsorted_list_is_scipys_P_A_Pt(cuda):
    rng = np.random.default_rng(8)
    n, m = 301, 2500
    cells = rng.choice(n * n, size=m, replace=False)                        # no pair twice, in no order
    row, col = cells // n, cells % n
    val = common.order_sensitive_weights(rng, m)
    assert (np.diff(cells) < 0).any()
    adj = io.coo_to_csr_device(row, col, val, n, device=cuda)
    a = sp.csr_matrix((val, (row, col)), shape=(n, n))
    assert np.array_equal(adj.rowptr.cpu().numpy(), a.indptr) and np.array_equal(adj.col.cpu().numpy(), a.indices)
    assert np.array_equal(common.bits(adj.val.cpu().numpy()), common.bits(a.data))
    order = rng.permutation(n)
    rp, cc, vv = reorder.permute_csr(adj.rowptr, adj.col, adj.val, torch.from_numpy(order).to(cuda))
    Q = sp.coo_matrix((np.ones(n, np.float32), (order, np.arange(n))), shape=(n, n)).tocsr()
    want = (Q @ a @ Q.T).tocsr()
    want.sort_indices()
    direct = sp.csr_matrix((val, (order[row], order[col])), shape=(n, n))
    assert want.nnz == direct.nnz == m and np.array_equal(want.indices, direct.indices) and np.array_equal(common.bits(want.data), common.bits(direct.data))
    assert np.array_equal(rp.cpu().numpy(), want.indptr) and np.array_equal(cc.cpu().numpy(), want.indices)
    assert np.array_equal(common.bits(vv.cpu().numpy()), common.bits(want.data))
    assert not np.array_equal(want.indptr, a.indptr)

"""Label propagation and the row permutation on a real MI355X (csrc/sgl_reorder.hip: sgl_reorder_lpa_round, sgl_reorder_community,
sgl_csr_permute_rows): run with `-m gpu`.

The reference is the numpy statement of the per-node rule in reorder_common -- independent of the kernel, sampling included -- on rows
whose neighbour labels are laid out so that the sample decides (tests/test_reorder_cpu.py holds that condition), and numpy fancy
indexing for the permutation.  Everything is integers and copied bits: every comparison is exact."""
import numpy as np
import pytest
import torch

import reorder_common as common
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd import reorder

pytestmark = pytest.mark.gpu

POISON = -7


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def one_round(cuda, blk, rnd, last, count=True):
    """(new labels of the block, *d_moved) of one call of sgl_reorder_lpa_round; the output has poisoned words behind it"""
    n = blk["n_local"]
    rowptr, labels = up(blk["rowptr"], cuda), up(blk["labels"], cuda)
    col = up(blk["col"], cuda) if len(blk["col"]) else torch.zeros(1, dtype=torch.int32, device=cuda)
    out = torch.full((n + 8,), POISON, dtype=torch.int32, device=cuda)
    moved = torch.zeros(1, dtype=torch.int64, device=cuda)
    dev._call(cuda, "sgl_reorder_lpa_round", _lib.ptr(rowptr), _lib.ptr(col), n, blk["row0"], blk["n_global"], _lib.ptr(labels), _lib.ptr(out),
              rnd, last, _lib.ptr(moved) if count else None)
    torch.cuda.synchronize()
    assert bool((out[n:] == POISON).all()) and np.array_equal(labels.cpu().numpy(), blk["labels"])     # nothing behind the block; labels only read
    return out[:n].cpu().numpy(), int(moved.item())


@pytest.mark.parametrize("row0", common.ROW0S)
@pytest.mark.parametrize("name", common.BLOCK_CASES)
def test_one_round_on_constructed_labels(cuda, name, row0):
    blk = common.block_case(name, row0)
    for rnd, last in common.ROUNDS:
        want, want_moved = common.lpa_round_reference(blk["rowptr"], blk["col"], blk["labels"], rnd, last, row0)
        got, moved = one_round(cuda, blk, rnd, last)
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, [(blk["names"][k], int(got[k]), int(want[k])) for k in wrong[:5]]
        assert got.dtype == np.int32 and moved == want_moved, (rnd, last)
    got, moved = one_round(cuda, blk, 5, 1, count=False)                # without a counter: the same labels
    assert np.array_equal(got, common.lpa_round_reference(blk["rowptr"], blk["col"], blk["labels"], 5, 1, row0)[0]) and moved == 0


@pytest.fixture(scope="module")
def planted():
    m = common.planted_graph()
    assert m.shape[0] == 3000 and np.diff(m.indptr).max() > 2 * common.SAMPLE
    return m


@pytest.mark.parametrize("rounds", [1, 8])
def test_community_order_equals_the_rounds_of_the_reference(cuda, planted, rounds):
    m = planted
    n = m.shape[0]
    want, n_comm, moved = common.community_order_from_rounds(m.indptr, m.indices, n, rounds=rounds)
    order, text = reorder.community_order(up(m.indptr.astype(np.int64), cuda), up(m.indices.astype(np.int32), cuda), n, rounds=rounds)
    assert order.dtype == torch.int64 and np.array_equal(order.cpu().numpy(), want)
    assert text == common.info_text(n_comm, rounds, moved)
    assert np.array_equal(np.sort(want), np.arange(n)) and (rounds == 1 or n_comm < n // 10)


def raw_permute(cuda, rowptr, col, val, perm, entries=True):
    """sgl_csr_permute_rows through the raw ABI on poisoned outputs; entries=False: NULL col and val, the row pointer only"""
    n, nnz = len(rowptr) - 1, len(col)
    d = [up(rowptr, cuda), up(col, cuda) if nnz else torch.zeros(1, dtype=torch.int32, device=cuda),
         up(val, cuda) if nnz else torch.zeros(1, dtype=torch.float32, device=cuda),
         up(perm, cuda) if n else torch.zeros(1, dtype=torch.int32, device=cuda)]
    out_rowptr = torch.full((n + 1 + 8,), POISON, dtype=torch.int64, device=cuda)
    out_col = torch.full((nnz + 8,), POISON, dtype=torch.int32, device=cuda)
    out_val = torch.full((nnz + 8,), POISON, dtype=torch.int32, device=cuda)
    dev._call(cuda, "sgl_csr_permute_rows", _lib.ptr(d[0]), _lib.ptr(d[1]) if entries else None, _lib.ptr(d[2]) if entries else None, n,
              _lib.ptr(d[3]), _lib.ptr(out_rowptr), _lib.ptr(out_col), _lib.ptr(out_val))
    torch.cuda.synchronize()
    assert bool((out_rowptr[n + 1:] == POISON).all()) and bool((out_col[nnz:] == POISON).all()) and bool((out_val[nnz:] == POISON).all())
    return out_rowptr[:n + 1].cpu().numpy(), out_col[:nnz].cpu().numpy(), out_val[:nnz].cpu().numpy().view(np.float32)


@pytest.mark.parametrize("n", common.PERMUTE_NS)
def test_permute_rows_is_fancy_indexing(cuda, n):
    rowptr, col, val = common.permute_matrix(n)
    for name, perm in common.permutations(n).items():
        want = common.permute_rows_reference(rowptr, col, val, perm)
        got = raw_permute(cuda, rowptr, col, val, perm)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), name
        only = raw_permute(cuda, rowptr, col, val, perm, entries=False)       # the row pointer alone: nothing else is touched
        assert np.array_equal(only[0], want[0]), name
        assert (only[1] == POISON).all() and (only[2].view(np.int32) == POISON).all(), name
        through = dev.permute_rows(up(rowptr, cuda), up(col, cuda), up(val, cuda), up(perm, cuda))
        assert np.array_equal(through[0].cpu().numpy(), want[0]) and np.array_equal(through[1].cpu().numpy(), want[1]), name
        assert np.array_equal(through[2].cpu().numpy().view(np.uint32), want[2].view(np.uint32)), name


def test_permute_rows_of_an_empty_matrix(cuda):
    rowptr, col, val, perm = np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int32)
    for entries in (True, False):
        got = raw_permute(cuda, rowptr, col, val, perm, entries=entries)
        assert got[0].tolist() == [0] and len(got[1]) == len(got[2]) == 0
    through = dev.permute_rows(up(rowptr, cuda), up(col, cuda), up(val, cuda), up(perm, cuda))      # an empty tensor's pointer is NULL
    assert through[0].cpu().tolist() == [0] and through[1].numel() == through[2].numel() == 0
    hollow = dev.permute_rows(torch.zeros(4, dtype=torch.int64, device=cuda), up(col, cuda), up(val, cuda), up(np.array([2, 0, 1], np.int32), cuda))
    assert hollow[0].cpu().tolist() == [0, 0, 0, 0]                     # rows without entries

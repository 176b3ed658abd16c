"""CPU-side checks of the reorder tests' own reference (reorder_common): the numpy statement of lpa_round_kernel's per-node rule against
the tensor code of sgl_amd.reorder.community_order_reference, and the condition under which the GPU tests can see the kernel's
sampling of long rows at all -- on a random community graph the sample almost never changes a label, so the rows are constructed."""
import numpy as np
import pytest
import torch

import reorder_common as common
from sgl_amd.reorder import _mix, community_order_reference


def tensor_code(m, rounds):
    order, text = community_order_reference(torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int32)), m.shape[0],
                                            rounds=rounds)
    return order.numpy(), text


@pytest.mark.parametrize("rounds", [1, 2, 8])
def test_every_neighbour_counted_equals_the_tensor_code_on_a_graph_with_hubs(rounds):
    m = common.planted_graph(n=1200, bs=60, hubs=2, hub_deg=700, seed=3)
    assert np.diff(m.indptr).max() > 2 * common.SAMPLE
    order, n_comm, moved = common.community_order_from_rounds(m.indptr, m.indices, m.shape[0], rounds=rounds, sample=None)
    want, text = tensor_code(m, rounds)
    assert np.array_equal(order, want) and text == common.info_text(n_comm, rounds, moved)


def test_sampled_rule_equals_the_tensor_code_when_no_row_is_long():
    m = common.planted_graph(n=1200, bs=60, hubs=0, seed=4)
    assert 10 < np.diff(m.indptr).max() <= common.SAMPLE
    order, n_comm, moved = common.community_order_from_rounds(m.indptr, m.indices, m.shape[0], rounds=8, sample=common.SAMPLE)
    want, text = tensor_code(m, 8)
    assert np.array_equal(order, want) and text == common.info_text(n_comm, 8, moved)
    assert np.array_equal(np.sort(order), np.arange(1200)) and 5 < n_comm < 100


def test_activity_hash_is_the_tensor_codes_and_wraps_in_64_bits():
    ids = torch.arange(5000, dtype=torch.int64)
    for rnd in (0, 1, 2, 7, 63):
        want = ((_mix(ids, rnd * 2654435761 + 12345) & 1) == (rnd & 1)).numpy()
        got = np.array([common.lpa_active(i, rnd, 0) for i in range(5000)])
        assert np.array_equal(got, want) and 0.4 < got.mean() < 0.6
    assert all(common.lpa_active(i, 3, 1) for i in range(100))
    assert (5000 * 0x9E3779B97F4A7C15) >> 64 > 0                       # the product leaves 64 bits for these ids: the wrap-around is exercised


def test_the_sample_decides_every_long_constructed_row():
    """for every row above 256 neighbours of the `sampled` case the 256 sampled positions and the full count give different labels;
    the row of 511 in the layout A at 0 ... 255, B at 256 ... 510 gives A either way (256 against 255) and sits among the short rows"""
    for row0 in common.ROW0S:
        blk = common.block_case("sampled", row0)
        deg = np.diff(blk["rowptr"])
        assert sorted(deg.tolist()) == [257, 511, 512, 513, 768, 1000]
        sampled, _ = common.lpa_round_reference(blk["rowptr"], blk["col"], blk["labels"], 5, 1, row0, common.SAMPLE)
        full, _ = common.lpa_round_reference(blk["rowptr"], blk["col"], blk["labels"], 5, 1, row0, None)
        print(list(zip(blk["names"], sampled.tolist(), full.tolist())))
        assert (sampled != full).all()
    blk = common.block_case("short", 0)
    k = blk["names"].index("deg511 as in the layout A 0-255, B 256-510")
    for sample in (common.SAMPLE, None):
        assert common.lpa_round_reference(blk["rowptr"], blk["col"], blk["labels"], 5, 1, 0, sample)[0][k] == common.A


def wrong_round(blk, row0, variant):
    """the per-node rule with one line of the sampling wrong (last round: everybody active).  Reads beyond a row stay inside the array."""
    rowptr, col, labels = blk["rowptr"], blk["col"].astype(np.int64), blk["labels"]
    out = np.empty(len(rowptr) - 1, dtype=np.int32)
    for i in range(len(out)):
        p0, deg = int(rowptr[i]), int(rowptr[i + 1] - rowptr[i])
        if deg == 0:
            out[i] = labels[row0 + i]
            continue
        length, step = min(deg, 256), max(1, deg // 256)
        if variant == "step rounded up":
            step = (deg + 255) // 256
        if variant == "one position short":
            length = max(1, length - 1)
        start = 1 if variant == "starts at the second entry" and deg > 1 else 0
        pos = np.minimum(p0 + start + step * np.arange(length), len(col) - 1)
        seen, count = np.unique(labels[col[pos]], return_counts=True)
        out[i] = seen[np.argmax(count)] if variant != "ties to the larger label" else seen[len(count) - 1 - np.argmax(count[::-1])]
    return out


@pytest.mark.parametrize("variant", ["step rounded up", "one position short", "starts at the second entry", "ties to the larger label"])
def test_a_wrong_sampling_line_changes_the_constructed_rows(variant):
    """what a subtly wrong kernel would return, emulated on the CPU: it differs from the reference on the constructed rows -- while
    the whole-matrix-against-row-blocks test of the kernel with itself could not notice"""
    hit = 0
    for name in ("sampled", "short"):
        blk = common.block_case(name, 0)
        right, _ = common.lpa_round_reference(blk["rowptr"], blk["col"], blk["labels"], 5, 1, 0)
        assert np.array_equal(wrong_round(blk, 0, "none"), right)
        hit += int((wrong_round(blk, 0, variant) != right).sum())
    assert hit >= 2, variant


def test_constructed_blocks_cover_their_shapes():
    assert [common.block_case(f"n{k}", 0)["n_local"] for k in (1, 2, 3, 4, 5, 1023)] == [1, 2, 3, 4, 5, 1023]
    blk = common.block_case("n5", 37)
    assert np.diff(blk["rowptr"]).tolist() == [64, 0, 65, 4, 256] and blk["row0"] == 37
    short = common.block_case("short", 0)
    assert {1, 0, 64, 65, 255, 256} <= set(np.diff(short["rowptr"]).tolist())
    for name in common.BLOCK_CASES:
        for row0 in common.ROW0S:
            blk = common.block_case(name, row0)
            assert blk["labels"].dtype == np.int32 and 0 <= blk["labels"].min() and blk["labels"].max() < blk["n_global"]
            assert blk["col"].dtype == np.int32 and blk["col"].max(initial=0) < blk["n_global"] and row0 + blk["n_local"] <= blk["n_global"]
            new, moved = common.lpa_round_reference(blk["rowptr"], blk["col"], blk["labels"], 5, 1, row0)
            assert moved == int((new != blk["labels"][row0:row0 + blk["n_local"]]).sum())
    # the ties: who moves and who stays
    new, moved = common.lpa_round_reference(short["rowptr"], short["col"], short["labels"], 5, 1, 0)
    at = {n: k for k, n in enumerate(short["names"])}
    assert new[at["tie of two, node moves"]] == common.B and new[at["tie of two, own label the larger: moves"]] == common.B
    assert new[at["tie of two, own label the smaller: stays"]] == common.B == short["labels"][at["tie of two, own label the smaller: stays"]]
    assert new[at["tie of four"]] == common.D and new[at["tie across three slots"]] == common.C and new[at["tie across four slots"]] == common.D
    assert new[at["one label per position"]] == 100 and new[at["majority in the last slot"]] == common.A
    assert new[at["empty row between full ones"]] == 9
    # half of the nodes may move in a round that is not the last
    for rnd, last in common.ROUNDS[:3]:
        new, moved = common.lpa_round_reference(short["rowptr"], short["col"], short["labels"], rnd, last, 0)
        idle = [k for k in range(short["n_local"]) if not common.lpa_active(k, rnd, last)]
        assert 0 < len(idle) < short["n_local"] and all(new[k] == short["labels"][k] for k in idle)


def test_permute_reference_is_fancy_indexing():
    for n in common.PERMUTE_NS + (0,):
        rowptr, col, val = common.permute_matrix(n) if n else (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
        for name, perm in common.permutations(n).items():
            assert np.array_equal(np.sort(perm), np.arange(n))
            out_rowptr, out_col, out_val = common.permute_rows_reference(rowptr, col, val, perm)
            assert out_rowptr[-1] == rowptr[-1] and len(out_col) == len(col)
            for k in (0, n // 2, n - 1) if n else ():
                a, b = rowptr[perm[k]], rowptr[perm[k] + 1]
                assert np.array_equal(out_col[out_rowptr[k]:out_rowptr[k + 1]], col[a:b])
                assert np.array_equal(out_val[out_rowptr[k]:out_rowptr[k + 1]].view(np.uint32), val[a:b].view(np.uint32))
    assert set(np.diff(common.permute_matrix(8)[0]).tolist()) == set(common.PERMUTE_LENGTHS) <= set(np.diff(common.permute_matrix(1025)[0]).tolist())

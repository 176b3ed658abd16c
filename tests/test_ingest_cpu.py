"""CPU-side checks of the ingest tests' own reference (ingest_common, oracle.coo_to_csr) against scipy, and the conditions under which
the GPU tests of csrc/sgl_ingest.hip can notice a wrong summation order at all.

What scipy does and what the contract therefore is: csr_matrix((w, (row, col))) sorts every row's entries by column with an UNSTABLE
sort and then folds equal columns left to right.  A pair stored once or twice comes out with the bits of the storage-order sum
(a + b = b + a).  A pair stored three times or more may be folded in another order: with weights whose magnitudes span 2^-20 ... 2^20,
scipy 1.15.3 differed from the storage-order float32 sum in 93 of 1704 runs of an edge list of 4000 entries, every one of them a run
of three or more.  So the library's contract is the storage-order sequential float32 sum, bit-equal to scipy wherever a pair occurs
at most twice; the structure (row pointer, columns, number of entries, zeros that stay entries) is scipy's everywhere."""
import numpy as np
import pytest

import ingest_common as common
import oracle


def plain_loop(z, n_cols=None):
    with np.errstate(invalid="ignore", over="ignore"):
        return oracle.coo_to_csr(z["row"], z["col"], z["val"], z["n_rows"], z["n_cols"] if n_cols is None else n_cols)


@pytest.mark.parametrize("name", common.ZOO_NAMES)
def test_fast_reference_equals_the_plain_loop(name):
    z = common.BY_NAME[name]
    indptr, indices, values, nnz, _ = common.reference(name)
    p, i, v = plain_loop(z)
    assert np.array_equal(indptr, p) and indptr.dtype == p.dtype == np.int64
    assert np.array_equal(indices, i) and indices.dtype == i.dtype == np.int32
    assert common.same_values(values, v) and nnz == len(v) == indptr[-1]
    if name == "one_key_100000":                                       # the long-run path of the fast form is the one taken here
        assert nnz == 1 and common.reference(name)[4][0] == 100_000 > common.LONG_RUN


def test_accumulate_is_the_sequential_sum_and_pairwise_is_not():
    v = common.order_sensitive_weights(np.random.default_rng(1), 5000)
    acc = np.float32(v[0])
    for x in v[1:]:
        acc = np.float32(acc + x)
    assert np.add.accumulate(v, dtype=np.float32)[-1].view(np.uint32) == acc.view(np.uint32)
    assert np.add.reduce(v, dtype=np.float32).view(np.uint32) != acc.view(np.uint32)      # numpy's pairwise sum: another order, other bits


def test_order_sensitive_weights_are_what_they_say():
    v = common.order_sensitive_weights(np.random.default_rng(2), 20000)
    assert v.dtype == np.float32 and np.isfinite(v).all() and (v != 0).all()
    mant, exp = np.frexp(np.abs(v).astype(np.float64))                 # |v| = mant * 2^exp, mant in [0.5, 1)  <=>  U(1, 2) * 2^(exp - 1)
    assert set(np.unique(exp - 1).tolist()) <= set(range(-20, 22)) and {-20, 0, 20} <= set((exp - 1).tolist())
    assert 0.45 < (v < 0).mean() < 0.55


@pytest.mark.parametrize("name", common.ZOO_NAMES)
def test_zoo_conditions(name):
    """the summation order shows: reversing the storage order inside the runs changes at least one run of three or more in every case
    that has such runs, and no run of one or two; every case meant to have long runs has them; runs sit where the case puts them"""
    z = common.BY_NAME[name]
    indptr, indices, values, nnz, lengths = common.reference(name)
    rev = common.coo_to_csr_reference(z["row"], z["col"], z["val"], z["n_rows"], z["n_cols"], reverse=True)
    assert np.array_equal(rev[0], indptr) and np.array_equal(rev[1], indices) and rev[3] == nnz
    diff = common.changed(rev[2], values)
    print(name, "entries", len(z["row"]), "runs", nnz, "runs >= 3:", int((lengths >= 3).sum()), "changed by reversal:", int(diff.sum()))
    assert not diff[lengths <= 2].any()
    if z["long_runs"]:
        assert (lengths >= 3).any()
    if (lengths >= 3).any():
        assert diff[lengths >= 3].any()
    starts = np.cumsum(lengths) - lengths
    for at, length in z["runs_at"].items():
        k = int(np.flatnonzero(starts == at)[0])
        assert lengths[k] == length
    assert z["row"].dtype == z["col"].dtype == np.int64 and z["val"].dtype == np.float32
    assert len(z["row"]) == len(z["col"]) == len(z["val"]) == lengths.sum()


def test_zoo_covers_what_it_is_for():
    by = common.BY_NAME
    assert {len(by[f"nnz{k}"]["row"]) for k in (1, 255, 256, 257, 1025)} == {1, 255, 256, 257, 1025}
    assert common.reference("run5_at_254")[4][254] == 5                # sorted positions 254 ... 258: two blocks of 256 threads
    for n_rows in (1, 2, 3, 4, 5, 1 << 16, (1 << 16) + 1, (1 << 20) + 1):
        z = by[f"rows{n_rows}_ends"]
        assert z["n_rows"] == n_rows and {0, n_rows - 1} == set(z["row"].tolist()) and {0, z["n_cols"] - 1} <= set(z["col"].tolist())
        if n_rows >= 3:
            z = by[f"rows{n_rows}_inside"]
            deg = np.diff(common.reference(z["name"])[0])
            assert deg[0] == 0 and deg[-1] == 0 and deg.sum() > 0 and (n_rows < 5 or (deg[1:-1] == 0).any())
    for name, (n_rows, n_cols) in (("tall_1_column", (4, 1)), ("wide_7_columns", (3, 7)), ("columns_to_2^31-3", (5, (1 << 31) - 2))):
        z = by[name]
        assert (z["n_rows"], z["n_cols"]) == (n_rows, n_cols) and {0, n_cols - 1} <= set(z["col"].tolist())
    # storage order of the interleaved cases: between two members of a run lie entries of other pairs
    z = by["interleaved"]
    key = z["row"] * z["n_cols"] + z["col"]
    assert all(key[i] != key[i + 1] for i in range(len(key) - 1)) and len(set(key.tolist())) == 4
    v = common.reference("special_values")[2]
    b = common.bits(v).tolist()
    assert b.count(0x80000000) == 2 and b.count(0) == 2 and np.isnan(v).sum() == 2 and np.isinf(v).sum() == 1
    assert common.reference("special_values")[3] == 8                  # the sums that cancel to zero are still entries
    for name in ("empty_0_rows", "empty_5_rows"):
        indptr, indices, values, nnz, _ = common.reference(name)
        assert nnz == 0 and len(indices) == len(values) == 0 and indptr.tolist() == [0] * (by[name]["n_rows"] + 1)


@pytest.mark.parametrize("name", common.ZOO_NAMES)
def test_reference_against_scipy(name):
    """structure and number of entries everywhere; the values on every run of at most two"""
    z = common.BY_NAME[name]
    indptr, indices, values, nnz, lengths = common.reference(name)
    a = common.scipy_csr(z)
    assert a.nnz == nnz and np.array_equal(a.indptr, indptr) and np.array_equal(a.indices, indices)
    short = lengths <= 2
    assert common.same_values(np.asarray(a.data, dtype=np.float32)[short], values[short])
    print(name, "scipy differs on", int(common.changed(a.data, values).sum()), "of", int((~short).sum()), "runs of three or more")


def test_oracle_equals_the_reference_on_g7(goldens):
    g7 = goldens.npz("g7_ingest")
    n = int(g7["n"])
    indptr, indices, values, nnz = common.coo_to_csr_reference(g7["row"], g7["col"], g7["data"], n, n)
    p, i, v = oracle.coo_to_csr(g7["row"], g7["col"], g7["data"], n)
    assert np.array_equal(p, indptr) and np.array_equal(i, indices) and np.array_equal(common.bits(v), common.bits(values))
    assert nnz == len(g7["indices"]) and np.array_equal(indptr, g7["indptr"]) and np.array_equal(indices, g7["indices"])
    lengths = common.run_lengths(g7["row"], g7["col"], n)
    short = lengths <= 2
    assert np.array_equal(common.bits(values[short]), common.bits(g7["values"][short]))     # the golden is scipy's: exact on runs <= 2
    assert (values != g7["values"]).sum() <= 2 and (lengths[values != g7["values"]] >= 3).all()


def test_wrong_orders_are_told_apart(goldens):
    """What a wrong build would give, emulated in the reference: a key order that is not stable (the members of a run reversed) changes
    the values of the zoo, while G7's weights in [0.1, 2] with the tolerance the suite used before let it pass."""
    g7 = goldens.npz("g7_ingest")
    n = int(g7["n"])
    wrong = common.coo_to_csr_reference(g7["row"], g7["col"], g7["data"], n, n, reverse=True)[2]
    assert (wrong != g7["values"]).sum() <= 2 and np.allclose(wrong, g7["values"], rtol=3e-7, atol=0)       # the old check: passes
    assert not np.array_equal(wrong, oracle.coo_to_csr(g7["row"], g7["col"], g7["data"], n)[2])              # the tightened one: fails
    hit = [n for n in common.ZOO_NAMES if common.changed(
        common.coo_to_csr_reference(*(common.BY_NAME[n][k] for k in ("row", "col", "val", "n_rows", "n_cols")), reverse=True)[2],
        common.reference(n)[2]).any()]
    assert {"nnz255", "nnz1025", "one_key_300", "one_key_100000", "run5_at_254", "run4_at_255", "run4_at_256", "interleaved",
            "interleaved_descending", "tall_1_column", "wide_7_columns", "columns_to_2^31-3", "special_values", "sharded_square"} <= set(hit)

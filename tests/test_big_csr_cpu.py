"""What test_gpu_big_csr.py rests on, checked without a GPU: the formulas of big_csr_common.py against scipy and the committed oracles at
a size of a few thousand rows, the property that makes the big cases able to see a truncated position ("not blind"), the SpMM plan's
arithmetic on the full-size row pointers, the caps the sources state, and the list of covered entry points against the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

import big_csr_common as big
import csr_merge_common
import edge_split_common
import reorder_common
from oracle import ref_ops as oracle
from sgl_amd import _lib

INT32_MAX = np.iinfo(np.int32).max


def small(kind):
    """the same generator at a few thousand rows: every feature of the big instances (offsets that fall off either edge, the three
    width classes, the short first row, a diagonal that only long rows store) at a size scipy holds"""
    if kind == "symmetric":
        k = np.arange(16, dtype=np.int64)
        s = 7 * k + 1 + k % 3
        return big.BigCSR(2500, np.concatenate((-s[::-1], s)), 32, (), symmetric=True)
    k = np.arange(400, dtype=np.int64)
    return big.BigCSR(3001, 5 * k - 300 + k % 3, 32, ((53, 3, 0), (53, 7, 1), (211, 11, 150)), first=20)


@pytest.fixture(scope="module", params=["directed", "symmetric"])
def graph(request):
    g = small(request.param)
    return g, g.scipy()


def test_rows_columns_and_rowptr_equal_a_scipy_matrix(graph):
    g, a = graph
    assert a.has_canonical_format and a.nnz == g.nnz and np.array_equal(a.indptr, g.rowptr)
    lengths = set(np.diff(g.rowptr).tolist())
    assert ({0, 1, 150, 32, 20} <= lengths) if not g.symmetric else (32 in lengths and min(lengths) < 32)
    csc = a.tocsc()
    for j in range(g.n):
        i, v, p = g.column(j)
        assert np.array_equal(i, csc.indices[csc.indptr[j]:csc.indptr[j + 1]]), j
        assert csr_merge_common.same_bits(v, csc.data[csc.indptr[j]:csc.indptr[j + 1]].astype(np.float32)), j
        assert np.array_equal(a.indices[p], np.full(len(p), j)), j
    assert np.array_equal(big.column_lengths(g).numpy(), np.diff(csc.indptr))
    if g.symmetric:
        assert (a != a.T).nnz == 0
    else:
        assert (a != a.T).nnz > 0 and 0 < a.diagonal().astype(bool).sum() < g.n
    for mode in ("hash", "pos"):
        rp, col, val = g.generate("cpu", mode=mode, chunk=1000)                    # the device generator, here on the CPU
        assert np.array_equal(rp.numpy(), g.rowptr) and np.array_equal(col.numpy(), a.indices)
        want = a.data if mode == "hash" else (np.arange(g.nnz) & 0x7FFFFFFF).astype(np.uint32).view(np.float32)
        assert csr_merge_common.same_bits(val.numpy(), want.astype(np.float32))
    assert 0.5 <= a.data.min() and a.data.max() < 1 and len(np.unique(a.data)) > 0.99 * a.nnz / (2 if g.symmetric else 1)
    rng = np.random.RandomState(1)
    qi, qj = rng.randint(0, g.n, 20000), rng.randint(0, g.n, 20000)
    qi[:5000], qj[:5000] = np.repeat(np.arange(g.n), np.diff(g.rowptr))[::max(g.nnz // 5000, 1)][:5000], a.indices[::max(g.nnz // 5000, 1)][:5000]
    dense_pos = {(r, c): p for p, (r, c) in enumerate(zip(np.repeat(np.arange(g.n), np.diff(g.rowptr)).tolist(), a.indices.tolist()))}
    want = np.array([dense_pos.get(rc, -1) for rc in zip(qi.tolist(), qj.tolist())])
    assert np.array_equal(g.find(qi, qj), want) and (want >= 0).sum() >= 5000 and (want < 0).sum() > 5000
    for p in (0, 1, g.nnz // 2, g.nnz - 1):
        i, c, bits = g.entry_at(p)
        assert g.rowptr[i] <= p < g.rowptr[i + 1] and c == a.indices[p] and bits == a.data[p:p + 1].view(np.uint32)[0]


def sample(g):
    rows = sorted(set(g.near_rows().tolist()) | {g.n - 1, g.n // 2, 3, 7, 11, 64, 222})
    return np.asarray([r for r in rows if r < g.n], dtype=np.int64)


def test_sampled_row_products_equal_the_full_oracle(graph):
    g, a = graph
    rows = sample(g)
    x = np.random.RandomState(2).randn(g.n, 5).astype(np.float32)
    indptr, idx, vals, cols = g.sub_matrix(rows)
    assert csr_merge_common.same_bits(oracle.oracle_spmm(indptr, idx, vals, x[cols]), oracle.oracle_spmm(a.indptr, a.indices, a.data, x)[rows])
    for R, cut in ((1, 100), (4, 100), (8, -1)):
        assert csr_merge_common.same_bits(oracle.oracle_spmm_slots(indptr, idx, vals, x[cols], R, cut),
                                          oracle.oracle_spmm_slots(a.indptr, a.indices, a.data, x, R, cut, rows=rows))


@pytest.mark.parametrize("r,alpha", [(0.5, None), (0.3, None), (0.5, 0.15)])
def test_sampled_row_normalisation_equals_the_full_oracle(graph, r, alpha):
    g, a = graph
    rows = sample(g)
    ptr, col, val = oracle.sym_norm_csr(a.indptr, a.indices, a.data, g.n, r, alpha)
    for j, (c, v) in zip(rows, big.norm_rows_reference(g, rows, r, alpha)):
        assert np.array_equal(c, col[ptr[j]:ptr[j + 1]]), j
        assert csr_merge_common.same_bits(v, val[ptr[j]:ptr[j + 1]]), j


def test_sampled_row_merge_lookup_and_label_round_equal_their_references(graph):
    g, a = graph
    rows = sample(g)
    rng = np.random.RandomState(3)
    brows = {int(i): np.unique(np.concatenate(([i], rng.randint(0, g.n, 3), g.row(i)[0][:2]))) for i in rows[::2]}
    bi = np.concatenate([np.full(len(c), i) for i, c in brows.items()])
    bj = np.concatenate(list(brows.values()))
    bv = (rng.rand(len(bi)) + 1).astype(np.float32)
    b = sp.csr_matrix((bv, (bi, bj)), shape=a.shape)
    b.sort_indices()
    for mode, name in ((csr_merge_common.SUM, "sum"), (csr_merge_common.KEEP, "keep")):
        indptr, idx, data, pa, pb = csr_merge_common.merge_reference(a, b, mode)
        for i in rows:
            c, bits, qa, qb = big.merge_row_reference(g, i, b.indices[b.indptr[i]:b.indptr[i + 1]], b.data[b.indptr[i]:b.indptr[i + 1]], name)
            s = slice(indptr[i], indptr[i + 1])
            assert np.array_equal(c, idx[s]) and np.array_equal(bits, data[s].view(np.uint32)) and np.array_equal(qa, pa[s]), (i, name)
            assert np.array_equal(np.where(qb >= 0, qb + b.indptr[i], -1), pb[s]), (i, name)
    pairs = edge_split_common.candidate_pairs(g.n, 9, 5, 4000)
    stored = edge_split_common.stored_set(a)
    free = (pairs[:, 0] != pairs[:, 1]) & (g.find(pairs[:, 0], pairs[:, 1]) < 0)
    key = np.where(free, pairs.min(1) * g.n + pairs.max(1), -1)
    assert np.array_equal(key, edge_split_common.candidate_keys(stored, g.n, pairs)) and (key < 0).any()
    labels = ((np.arange(g.n) // 7) % 19).astype(np.int32)
    for rnd, last in ((0, 0), (1, 0), (2, 1)):
        full, _ = reorder_common.lpa_round_reference(a.indptr, a.indices, labels, rnd, last)
        assert np.array_equal(big.lpa_rows_reference(g, rows, labels, rnd, last), full[rows]) and (full != labels).any()


# ---- the real sizes, from the formulas alone -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[("directed", "B"), ("directed", "A"), ("symmetric", "B")], ids=lambda p: f"{p[0]}-{p[1]}")
def full_size(request):
    kind, tier = request.param
    return big.instance(kind, tier), kind, tier


def test_sizes_and_sampled_rows_of_every_tier(full_size):
    g, kind, tier = full_size
    assert g.nnz >= big.TIERS[tier][0] and g.nnz < (1 << 32) + (1 << 24) and g.n < INT32_MAX
    if tier == "B":
        assert g.nnz < (1 << 32) - (1 << 22)                                      # below the caps of the normaliser and the ingest
    bounds = big.boundaries(tier)
    near, far = g.near_rows(), g.far_rows(bounds)
    assert len(near) == 64 and g.rowptr[near + 1].max() < (1 << 30)
    assert len(far) >= 256 and len(set(far.tolist())) == len(far)
    strad = [g.straddler(b) for b in bounds]
    assert all(s is not None and s in far for s in strad)
    beyond = far[g.rowptr[far] >= bounds[-1]]
    assert len(beyond) >= 256 and g.n - 1 in beyond
    classes = {g.row_class(int(i)) for i in beyond}
    assert classes >= ({"base", "last"} | ({0, 1, big.LONG} if kind == "directed" else set())), classes
    lengths = set(g.len[beyond].tolist())
    assert ({0, 1, 1024} <= lengths and max(lengths) > 2048) if kind == "directed" else (1024 in lengths and min(lengths) < 1024)
    if kind == "directed":
        assert {g.row_class(int(i)) for i in near} >= {"first", "base", 0, 1, big.LONG}
        assert g.len[0] == 700 and np.count_nonzero(g.rowptr[1:] % 1024 == 0) < g.n // 500    # row boundaries are no multiples of 1024


def test_a_truncated_position_reads_another_entry(full_size):
    """NOT BLIND: a kernel that keeps a position in 32 bits reads, for an entry at p beyond the boundary, the entry at p - 2^32
    (unsigned), p - 2^31 (the sign bit lost) or a negative address.  At every sampled far row the first, a middle and the last entry
    differ in (column, value) from both of those, in either value mode."""
    g, kind, tier = full_size
    bounds = big.boundaries(tier)
    far = g.far_rows(bounds)
    checked = 0
    for i in far.tolist():
        b, e = int(g.rowptr[i]), int(g.rowptr[i + 1])
        if e <= bounds[0]:
            continue
        for p in sorted({max(b, bounds[0]), (max(b, bounds[0]) + e) // 2, e - 1}):
            if p >= e:
                continue
            for mode in ("hash", "pos"):
                here = g.entry_at(p, mode)[1:]
                for back in (1 << 31, 1 << 32):
                    if p - back >= 0:
                        assert g.entry_at(p - back, mode)[1:] != here, (i, p, back, mode)
            if p < (1 << 32):
                assert np.int64(p).astype(np.int32) < 0
            else:
                assert int(np.int64(p).astype(np.uint32)) != p and tier == "A"
            checked += 1
    assert checked >= 2 * 256


@pytest.mark.parametrize("item_nnz,long_row_nnz", [(512, 2048), (64, 2048), (512, big.SMALL_LONG_ROW_NNZ), (512, -1)])
def test_plan_arithmetic_at_full_size(full_size, item_nnz, long_row_nnz):
    g, kind, tier = full_size
    lib = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(lib.sgl_plan_build(ctypes.byref(h), g.rowptr.ctypes.data_as(ctypes.c_void_p), g.n, item_nnz, long_row_nnz))
    counts = (ctypes.c_int64 * 8)()
    _lib.check(lib.sgl_plan_counts(h, counts))
    ni, npc, nl = counts[0], counts[1], counts[2]
    items = np.zeros(2 * ni, np.int32)
    pb, pl, pr = np.zeros(npc, np.int64), np.zeros(npc, np.int32), np.zeros(npc, np.int32)
    lr, lf = np.zeros(nl, np.int32), np.zeros(nl + 1, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.check(lib.sgl_plan_export(h, p(items), p(pb), p(pl), p(pr), p(lr), p(lf)))
    lib.sgl_plan_destroy(h)
    items = items.reshape(-1, 2).astype(np.int64)
    cut = g.len > long_row_nnz if long_row_nnz > 0 else np.zeros(g.n, bool)
    assert counts[5] == g.n and nl == cut.sum() and np.array_equal(lr, np.nonzero(cut)[0])
    assert npc == (-(-g.len[cut] // long_row_nnz)).sum() if long_row_nnz > 0 else npc == 0
    # items and long rows tile the rows, pieces tile every long row, together they tile [0, nnz)
    items = items[np.argsort(items[:, 0], kind="stable")]
    covered = np.zeros(g.n + 1, np.int64)
    np.add.at(covered, items[:, 0], 1)
    np.add.at(covered, items[:, 1], -1)
    np.add.at(covered, lr.astype(np.int64), 1)
    np.add.at(covered, lr.astype(np.int64) + 1, -1)
    assert np.all(np.cumsum(covered)[:-1] == 1)
    item_nnz_got = g.rowptr[items[:, 1]] - g.rowptr[items[:, 0]]
    assert item_nnz_got.max() < INT32_MAX and item_nnz_got.max() == counts[4] and (items[:, 1] - items[:, 0]).max() == counts[3] <= 63
    assert item_nnz_got.sum() + pl.astype(np.int64).sum() == g.nnz
    if npc:
        assert np.array_equal(pr, np.repeat(lr, np.diff(lf))) and lf[0] == 0 and lf[-1] == npc
        assert np.array_equal(pb[lf[:-1]], g.rowptr[lr]) and np.array_equal((pb + pl)[lf[1:] - 1], g.rowptr[lr.astype(np.int64) + 1])
        inner = np.ones(npc, bool)
        inner[lf[1:] - 1] = False
        assert np.all(pl[inner] == long_row_nnz) and np.all(pl > 0) and np.all(pl <= long_row_nnz)
        assert np.array_equal((pb + pl)[inner], pb[1:][inner[:-1]])
        assert pb.max() > big.boundaries(tier)[-1]                               # a piece that begins beyond 2^31 / 2^32 keeps its 64 bits


# ---- the caps the sources state --------------------------------------------------------------------------------------------------------
def refused(rc, *words):
    msg = _lib.last_error()
    assert rc != 0 and msg and all(w in msg for w in words), (rc, msg)


def test_the_caps_are_refused_by_name_without_a_gpu():
    lib = _lib.lib()
    keep = np.zeros(64, np.int64)
    q = ctypes.c_void_p(keep.ctypes.data)                                        # never dereferenced: the size check comes first
    out = ctypes.c_int64(0)
    U32 = (1 << 32) - 1
    refused(lib.sgl_coo_to_csr(8, 8, U32, q, q, q, q, q, q, ctypes.byref(out), None), "sgl_coo_to_csr", "2^32-1")
    refused(lib.sgl_norm_block_colsum(8, U32, q, q, q, None), "sgl_norm_block_colsum", "2^32")
    refused(lib.sgl_norm_execute(8, U32, q, q, q, 0.5, 0, 0.0, U32, q, q, q, None, None), "sgl_norm_execute", "2^32")
    refused(lib.sgl_norm_execute_lr(8, U32, q, q, q, q, q, 0, 0.0, U32, q, q, q, None, None), "sgl_norm_execute", "2^32")
    refused(lib.sgl_norm_block_build(8, 0, U32 - 4096, q, q, q, U32 - 4096, q, q, q, q, None), "sgl_norm_block_build", "2^32")
    refused(lib.sgl_norm_build_symcheck(8, U32 - 4096, q, q, q, U32 - 4096, q, q, q, q, q, None), "sgl_norm_block_build", "2^32")
    for name, args in (("sgl_csr_find", (q, q, 8, 1 << 31, q, 1, q, None)), ("sgl_edge_candidates", (q, q, 1 << 31, 1, 0, 1, q, q, None)),
                       ("sgl_csr_permute_rows", (q, q, q, INT32_MAX, q, q, q, q, None)),
                       ("sgl_reorder_lpa_round", (q, q, 8, 0, INT32_MAX, q, q, 0, 0, None, None))):
        refused(getattr(lib, name)(*args), name)


# ---- completeness ----------------------------------------------------------------------------------------------------------------------
CSR_PARAMETER = re.compile(r"\b(d_rowptr|a_rowptr|d_col|a_col|d_edges|d_pieces|d_inc_\w+)\b|sgl_csr_t\s*\*")


def csr_entry_points():
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = []
    for m in re.finditer(r"\b(?:int|void)\s+(\w+)\s*\(([^;{]*?)\)\s*;", text):
        if CSR_PARAMETER.search(m.group(2)):
            names.append(m.group(1))
    return names


def test_every_csr_entry_point_has_a_big_case_or_a_stated_exclusion():
    names = csr_entry_points()
    assert len(names) >= 37 and "sgl_edge_loss_grad_f32" in names and {"sgl_spmm_f32", "sgl_csr_merge_fill", "sgl_coo_to_csr", "sgl_norm_block_scale", "sgl_csr_find"} <= set(names)
    listed = set(big.COVERED) | set(big.EXCLUDED)
    assert not set(big.COVERED) & set(big.EXCLUDED)
    assert sorted(set(names) - listed) == [], "an entry point that takes a CSR or an entry list has no case in test_gpu_big_csr.py"
    assert all(hasattr(_lib.lib(), name) for name in listed)
    assert all(len(reason) > 40 for reason in big.EXCLUDED.values())
    source = open(os.path.join(ROOT, "tests", "test_gpu_big_csr.py")).read()
    tests = set(re.findall(r"^def (test_\w+)\(", source, flags=re.M))
    for name, cases in big.COVERED.items():
        assert cases and set(cases) <= tests, (name, cases)

"""The exact CPU model of the SpMM kernels' DEFAULT summation order (oracle.oracle_spmm_slots) pinned without a GPU: against the
strict chain, the fp64 product and the execution plan the library really builds; plus the helpers the GPU test
(test_gpu_spmm_order.py) relies on: the kernel-name parser and the restated dispatch / launch tables."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import oracle
from inputs import hash_matrix
from spmm_order_common import (TUNING_VALUES, compiled_variants, cut_rule, default_long_row_nnz, dense_graph, dispatch, medium_graph,
                               parse_kernel_name)
from test_gpu_bf16 import long_row_graph
from test_host_cpu import build_plan


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def graphs(goldens):
    out = {}
    for name in ("pl2000", "dir40", "sym64"):
        g = goldens.graph(name)
        ptr, col, val = oracle.sym_norm_csr(g.indptr, g.indices, g.data, g.shape[0], 0.5, None)
        out[name] = (np.asarray(ptr, np.int64), np.asarray(col, np.int32), val.astype(np.float32))
    for name, a in (("longrow", long_row_graph()), ("medium", medium_graph()), ("dense", dense_graph())):
        out[name] = (a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float32))
    return out


def test_test_graphs_have_the_promised_shape():
    for a, lo, hi in ((long_row_graph(), 0.0, 12.0), (medium_graph(), 12.0, 40.0), (dense_graph(), 40.0, 1e9)):
        deg = np.diff(a.indptr)
        assert a.has_canonical_format and a.shape[0] <= 2000
        assert lo <= a.nnz / a.shape[0] < hi, a.nnz / a.shape[0]
        assert (deg >= 900).sum() == 3 and (deg == 0).sum() > 0
        assert a.nnz < (1 << 18) and default_long_row_nnz(a.nnz) == 32


def test_one_slot_uncut_is_the_strict_chain(goldens):
    """R = 1 without cutting is the reference's sequential fmaf chain, bit for bit"""
    for name, (ptr, col, val) in graphs(goldens).items():
        n = len(ptr) - 1
        for d in (1, 16, 37):
            x = hash_matrix(n, d, seed=d + 3)
            want = oracle.oracle_spmm(ptr, col, val, x)
            for cut in (0, -1):
                assert np.array_equal(f32_bits(oracle.oracle_spmm_slots(ptr, col, val, x, 1, cut)), f32_bits(want)), (name, d, cut)


def test_order_matters_in_fp32_and_barely_in_bf16():
    """what makes the bit comparison a check of the ORDER: most fp32 elements change with R (so a wrong R cannot pass), while after
    the bf16 rounding only a small share still differs (that comparison guards the terms and the rounding)"""
    a = dense_graph()
    ptr, col, val = a.indptr.astype(np.int64), a.indices, a.data
    xb = torch.from_numpy(hash_matrix(a.shape[0], 16, seed=4)).to(torch.bfloat16)
    x = xb.float().numpy()
    strict = oracle.oracle_spmm(ptr, col, val, x)
    sb = torch.from_numpy(strict).to(torch.bfloat16).view(torch.int16).numpy()
    for R in (2, 4, 8):
        y = oracle.oracle_spmm_slots(ptr, col, val, x, R, 0)
        assert (f32_bits(y) != f32_bits(strict)).mean() > 0.5, R
        yb = oracle.oracle_spmm_slots_bf16(ptr, col, val, xb, R, 0)
        assert yb.dtype == torch.bfloat16 and np.array_equal(yb.view(torch.int16).numpy(), torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy())
        assert (yb.view(torch.int16).numpy() != sb).mean() < 0.02, R
    for R, other in ((2, 4), (4, 8), (8, 2)):
        assert (f32_bits(oracle.oracle_spmm_slots(ptr, col, val, x, R, 128)) != f32_bits(oracle.oracle_spmm_slots(ptr, col, val, x, other, 128))).mean() > 0.5
    assert (f32_bits(oracle.oracle_spmm_slots(ptr, col, val, x, 4, 32)) != f32_bits(oracle.oracle_spmm_slots(ptr, col, val, x, 4, 0))).any()


@pytest.mark.parametrize("R", [1, 2, 4, 8])
@pytest.mark.parametrize("cut", [0, 32, 128])
def test_every_slot_count_is_within_the_truth_bound(goldens, R, cut):
    """any R, cut or not, is an fp32 evaluation of the same sums: inside truth_report's bound (factor 2, the standing floor)
    against the fp64 product, with the strict chain as the fp32 reference"""
    for name, (ptr, col, val) in graphs(goldens).items():
        n = len(ptr) - 1
        a64 = sp.csr_matrix((val.astype(np.float64), col, ptr), shape=(n, n))
        for d in (5, 16, 100):
            x = hash_matrix(n, d, seed=d)
            rep = oracle.truth_report(oracle.oracle_spmm_slots(ptr, col, val, x, R, cut), oracle.oracle_spmm(ptr, col, val, x),
                                      a64 @ x.astype(np.float64))
            assert rep["ok"], (name, d, rep)


def test_empty_rows_leading_dimensions_and_row_subsets():
    a = dense_graph()
    ptr, col, val = a.indptr.astype(np.int64), a.indices, a.data
    n = a.shape[0]
    empty = np.flatnonzero(np.diff(ptr) == 0)
    assert len(empty) > 0
    x = hash_matrix(n, 24, seed=8)
    for R in (1, 2, 4, 8):
        for cut in (0, 32):
            y = oracle.oracle_spmm_slots(ptr, col, val, x, R, cut)
            assert not f32_bits(y[empty]).any()                                  # +0.0, not -0.0
            # a column window of a wider matrix (leading dimension > d) and a row subset against the full x
            assert np.array_equal(f32_bits(oracle.oracle_spmm_slots(ptr, col, val, x[:, 3:19], R, cut)), f32_bits(y[:, 3:19]))
            rows = np.array([n - 1, 3, int(empty[0]), 3, 0], np.int64)
            assert np.array_equal(f32_bits(oracle.oracle_spmm_slots(ptr, col, val, x, R, cut, rows=rows)), f32_bits(y[rows]))
    assert oracle.oracle_spmm_slots(ptr, col, val, x, 4, 32, rows=np.zeros(0, np.int64)).shape == (0, 24)
    with pytest.raises(ValueError):
        oracle.oracle_spmm_slots(ptr, col, val, x, 3, 0)
    with pytest.raises(IndexError):
        oracle.oracle_spmm_slots(ptr, col, val, x, 2, 0, rows=[n])


def test_model_by_hand():
    """five terms in R = 2 slots, cut at 4: piece 0 = (t0, t2 | t1, t3), piece 1 = (t4 | nothing); 0.f + p0 + p1"""
    v = np.array([1e8, 1.0, -1e8, 1.0, 0.5], np.float32)
    ptr, col = np.array([0, 5], np.int64), np.zeros(5, np.int32)
    x = np.ones((1, 1), np.float32)
    f = np.float32
    s0 = f(f(v[0]) + f(v[2]))
    s1 = f(f(v[1]) + f(v[3]))
    assert oracle.oracle_spmm_slots(ptr, col, v, x, 2, 4)[0, 0] == f(f(f(0) + f(s0 + s1)) + v[4]) == f(2.5)
    assert oracle.oracle_spmm_slots(ptr, col, v, x, 1, 0)[0, 0] == f(1.5)            # the chain loses the first 1.0
    assert oracle.oracle_spmm_slots(ptr, col, v, x, 2, 0)[0, 0] == f(2.5)            # slot 0 = 1e8 - 1e8 + 0.5, slot 1 = 2
    assert oracle.oracle_spmm_slots(ptr, col, v, x, 4, 0)[0, 0] == f(0.0)            # (fl(1e8 + 0.5) + 1) + (-1e8 + 1) = 1e8 - 1e8


@pytest.mark.parametrize("long_nnz", [3, 32, 128, 2048])
def test_exported_pieces_equal_the_cut_rule(long_nnz):
    """the plan sgl_plan_build really makes cuts the rows the model cuts, at the same places: a row of exactly long_row_nnz
    non-zeros is whole, one of long_row_nnz + 1 is two pieces (the second of length 1)"""
    rng = np.random.default_rng(long_nnz)
    n = 400
    deg = np.minimum(rng.lognormal(2.0, 1.5, n).astype(np.int64), 3 * long_nnz + 7)
    deg[[5, 6, 7, 8, 9]] = [long_nnz, long_nnz + 1, 2 * long_nnz, 2 * long_nnz + 1, 5 * long_nnz + 2]
    deg[[0, n - 1]] = [3 * long_nnz, long_nnz + 1]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    want = cut_rule(rowptr, long_nnz)
    assert not [w for w in want if w[0] == 5] and [w[2] for w in want if w[0] == 6] == [long_nnz, 1]
    for item_nnz in (16, 512):
        items, pb, pl, pr, lr, lf, counts = build_plan(rowptr, item_nnz, long_nnz)
        assert [(int(r), int(b), int(l)) for r, b, l in zip(pr, pb, pl)] == want
        assert list(lr) == sorted({w[0] for w in want}) and lf[0] == 0 and lf[-1] == len(want)
        for k, r in enumerate(lr):
            assert all(pr[q] == r for q in range(lf[k], lf[k + 1]))
    for never in (0, -1):
        assert cut_rule(rowptr, never) == [] and len(build_plan(rowptr, 64, -1)[1]) == 0


def test_default_cut_threshold_restatement():
    from sgl_amd import device as dev
    for nnz in (0, 1, (1 << 18) - 1, 1 << 18, (1 << 20) - 1, 1 << 20, (1 << 22) - 1, 1 << 22, 126_000_000):
        assert default_long_row_nnz(nnz) == dev.default_long_row_nnz(nnz)
    assert [default_long_row_nnz(v) for v in (1000, 1 << 18, 1 << 20, 1 << 22)] == [32, 128, 512, 2048]


def test_kernel_name_parser():
    cases = {
        "void (anonymous namespace)::spmm_bf16_kernel<8, 16, 1, 16>((anonymous namespace)::Bf16Args)": ("bf16", (8, 16, 1, 16)),
        "_ZN12_GLOBAL__N_116spmm_bf16_kernelILi8ELi16ELi1ELi16EEEvNS_8Bf16ArgsE": ("bf16", (8, 16, 1, 16)),
        "_ZN12_GLOBAL__N_116spmm_bf16_kernelILi1ELi64ELi4ELi2EEEvNS_8Bf16ArgsE.kd": ("bf16", (1, 64, 4, 2)),
        "void (anonymous namespace)::spmm_kernel<4, 64, 1, 32, true, false>((anonymous namespace)::SpmmArgs)": ("f32", (4, 64, 1, 32, 1)),
        "(anonymous namespace)::spmm_kernel<2,8,1,4,false,false>": ("f32", (2, 8, 1, 4, 0)),
        "_ZN12_GLOBAL__N_111spmm_kernelILi1ELi64ELi2ELi4ELb1ELb0EEEvNS_8SpmmArgsE": ("f32", (1, 64, 2, 4, 1)),
    }
    for name, want in cases.items():
        assert parse_kernel_name(name) == want, name
    for other in ("spmm_fixup_kernel(int const*, ...)", "_Z22spmm_bf16_fixup_kernelPKiS0_PKflPtliN12_GLOBAL__N_16AccEpiE",
                  "rowmap_check_kernel", "void at::native::vectorized_elementwise_kernel<4, ...>"):
        assert parse_kernel_name(other) is None, other


def test_restated_launch_tables_and_dispatch():
    bf, f32 = compiled_variants("bf16"), compiled_variants("f32")
    assert len(bf) == 64 and len(f32) == 102
    assert (8, 16, 1, 16) in bf and (4, 64, 1, 32, 1) in f32 and (8, 64, 1, 32) not in bf and (4, 32, 1, 32, 0) not in f32
    assert {v[3] for v in bf if v[2] == 2} == {2, 4} and {v[3] for v in bf if v[2] == 4} == {1, 2}
    A = 1 << 20                                                   # an aligned address
    # the products-shaped d = 100 hop at a 128-element pitch, >= 40 nnz per row
    assert dispatch("bf16", 100, 128, 128, A, A, False, 51.5) == [(0, 100, (4, 64, 1, 16))]
    assert dispatch("bf16", 128, 128, 128, A, A, False, 51.5) == [(0, 128, (8, 16, 1, 16))]
    assert dispatch("bf16", 104, 128, 128, A, A, False, 51.5) == [(0, 104, (8, 16, 1, 16))]
    assert dispatch("bf16", 104, 128, 128, A, A, False, 20.0) == [(0, 104, (8, 16, 1, 8))]
    assert dispatch("bf16", 104, 128, 128, A, A, True, 51.5) == [(0, 104, (8, 64, 1, 16))]
    assert dispatch("bf16", 104, 128, 128, A + 2, A, False, 51.5) == [(0, 104, (1, 64, 2, 4))]
    assert dispatch("bf16", 104, 128, 128, A + 4, A + 4, False, 5.0) == [(0, 104, (2, 64, 1, 4))]
    assert dispatch("bf16", 257, 257, 257, A, A, False, 5.0) == [(0, 256, (1, 64, 4, 2)), (256, 1, (1, 8, 1, 8))]
    assert dispatch("bf16", 104, 128, 128, A, A, False, 51.5, acc=(104, A + 4)) == [(0, 104, (1, 64, 2, 4))]
    assert dispatch("bf16", 104, 128, 128, A, A, False, 51.5, acc=(106, A + 8)) == [(0, 104, (2, 64, 1, 16))]
    assert dispatch("f32", 100, 128, 128, A, A, False, 51.5) == [(0, 100, (4, 64, 1, 16, 0))]
    assert dispatch("f32", 16, 16, 16, A, A, False, 51.5, {"spmm_nt": 1}) == [(0, 16, (4, 8, 1, 8, 1))]
    assert dispatch("f32", 16, 16, 16, A, A, True, 51.5, {"spmm_group": 32}) == [(0, 16, (4, 64, 1, 16, 0))]
    assert dispatch("f32", 16, 16, 16, A, A, False, 51.5, {"spmm_group": 32, "spmm_unroll": 4}) == [(0, 16, (4, 32, 1, 8, 0))]
    assert dispatch("f32", 1028, 1028, 1028, A, A, False, 5.0) == [(0, 1024, (4, 64, 4, 2, 0)), (1024, 4, (4, 8, 1, 8, 0))]
    assert dispatch("f32", 100, 100, 100, A, A, False, 5.0, {"spmm_vec": 2}, acc=(101, A)) == [(0, 100, (1, 64, 2, 4, 0))]


def test_library_launch_rule_and_default_thresholds_equal_the_restatements(tmp_path):
    """sgl::spmm_layout / default_item_nnz / default_long_row_nnz (csrc/sgl_core.cpp: pure host code), built with g++ into
    tests/native/spmm_layout_table.cpp and asked once: for both dtypes, every lane width and every width of the GPU test, strict
    or not, average row lengths on both sides of and exactly at the two thresholds, a matrix without rows (its average is 0 / 0:
    no threshold applies), and every value of the four launch keys one at a time, the library's (GROUP, NCH, U[, NT]) is
    spmm_order_common.dispatch's for every column slice and is a compiled variant; and the default cut threshold is the one
    restated in spmm_order_common and in sgl_amd.device at every step of the rule."""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    from sgl_amd import device as dev
    from test_gpu_spmm_order import WIDTHS
    gxx = shutil.which("g++")
    if gxx is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "spmm_layout_table")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "native", "spmm_layout_table.cpp"), os.path.join(ROOT, "sgl_amd", "csrc", "sgl_core.cpp"),
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    keys = ("spmm_group", "spmm_unroll", "spmm_waves", "spmm_nt")
    tunings = [{}] + [{k: v} for k in keys for v in TUNING_VALUES[k]]
    rows = ((6000, 1000), (25000, 1000), (60000, 1000), (12000, 1000), (40000, 1000), (0, 0))        # (nnz, n_rows)
    nnzs = ((1 << 18) - 1, 1 << 18, (1 << 20) - 1, 1 << 20, (1 << 22) - 1, 1 << 22, 10 ** 8 - 1, 10 ** 8)
    A = 1 << 20                                                   # an aligned address
    queries, want = [], []
    for dtype in ("f32", "bf16"):
        for W, widths in WIDTHS[dtype].items():
            for d in widths:
                for strict in (0, 1):
                    for nnz, n_rows in rows:
                        avg = nnz / n_rows if n_rows else float("nan")
                        for t in tunings:
                            for c0, dc, var in dispatch(dtype, d, d, d, A, A, bool(strict), avg, t):
                                assert var[0] == W, (dtype, d, var)
                                queries.append(f"{dtype} {dc // W} {strict} {nnz} {n_rows} " + " ".join(str(t.get(k, 0)) for k in keys))
                                waves = t.get("spmm_waves", 0)
                                want.append((dtype, var, waves if waves in (1, 2, 4) else 4))
    r = subprocess.run([exe], input="\n".join(queries + [str(v) for v in nnzs]) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(queries) + len(nnzs) and len(queries) > 10000
    seen = {"f32": set(), "bf16": set()}
    for q, (dtype, var, waves), (group, nch, u, nt, wv) in zip(queries, want, got):
        mine = (var[0], group, nch, u) + ((nt,) if dtype == "f32" else ())
        assert mine == var and wv == waves and (dtype == "f32" or nt == 0), (q, var, (group, nch, u, nt, wv))
        assert mine in compiled_variants(dtype), (q, mine)
        seen[dtype].add(mine)
    assert len(seen["f32"]) > 40 and len(seen["bf16"]) > 40                     # the queries reach the table, not one corner of it
    for nnz, (item_nnz, long_nnz) in zip(nnzs, got[len(queries):]):
        assert long_nnz == default_long_row_nnz(nnz) == dev.default_long_row_nnz(nnz), nnz
        # 8 192 items (one per resident wavefront) of at least 16 non-zeros, at most 256 below 10^8 non-zeros and 512 from there on
        assert item_nnz == min(512 if nnz >= 10 ** 8 else 256, max(16, nnz // 8192)), (nnz, item_nnz)
    assert [g[1] for g in got[len(queries):]] == [32, 128, 128, 512, 512, 2048, 2048, 2048]

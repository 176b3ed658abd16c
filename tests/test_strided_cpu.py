"""What test_gpu_strided_grids.py claims to test, proven without a GPU: by the restated launch arithmetic (strided_common.py) every
case of that file has more work than the cap in force, a workgroup that walks at least two units and -- unless one workgroup does
everything -- one that walks one fewer, and a partial last unit; the multi-tile cases restage their LDS tile in every batch; the
restated rules equal the library's host code (built with g++) and what the sources say; the tuning key loss_blocks exists; and the
share of near-tie rows of every new K9 input is within kmeans_common.MAX_LEFT_OUT, from the float64 reference alone."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import class_loss_common as zlc
import cluster_loss_common as clc
import kmeans_common as kc
import strided_common as sc
import edge_loss_common as elc
from edge_loss_common import hub_edges, plan_tables
from edge_scores_common import EDGES
from edge_scores_common import N_ROWS as EDGE_ROWS
from sgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(name):
    with open(os.path.join(ROOT, "sgl_amd", "csrc", name)) as f:
        return f.read()


def chunk_lists():
    """family -> {lane size: chunk counts of the compiled 64-lane instances}, as sgl_common.h states them: the lists that
    sgl::slice_instance reads and with_slice_instance (sgl_rows.h) dispatches"""
    text = source("sgl_common.h")
    found = re.findall(r"using (\w+)Slices = SliceFamily<Chunks<([\d, ]+)>, Chunks<([\d, ]+)>>;", text)
    assert len(found) == text.count("SliceFamily<Chunks<")                      # every family was read
    return {name: {4: tuple(int(v) for v in v4.split(",")), 1: tuple(int(v) for v in v1.split(","))} for name, v4, v1 in found}


def ok(g, what):
    assert g.work > g.cap, (what, g, "does not exceed the cap")
    assert g.rounds_max >= 2, (what, g)
    assert g.blocks == 1 or g.rounds_min == g.rounds_max - 1, (what, g, "every workgroup walks the same number of units")
    assert sc.strides(g) == (g.partial > 0), (what, g)


# ---- the caps and rules, as the sources state them ------------------------------------------------------------------------------------------
def test_caps_are_the_sources():
    km, cl, zl, el = source("sgl_kmeans.hip"), source("sgl_cluster_loss.hip"), source("sgl_class_loss.hip"), source("sgl_edge_loss.hip")
    assert f"constexpr int kMaxBlocks = {sc.CAP_K9};" in km and f"constexpr int kMaxBlocks = {sc.CAP_K12};" in cl
    assert "constexpr int64_t kMaxBlocks = (int64_t)1 << 20;" in zl and sc.CAP_K14 == 1 << 20
    assert f"constexpr int kMaxFoldBlocks = {sc.CAP_FOLD};" in el
    assert f"constexpr int kTileFloats = {sc.TILE_FLOATS};" in source("sgl_centres.h") and f"constexpr int kStep = {sc.K12_STEP};" in cl
    for text in (source("sgl_csr_select.hip"), source("sgl_csr_merge.hip")):
        assert f"if (blocks > {sc.CAP_CSR}) blocks = {sc.CAP_CSR};" in text and "rows_per_block = 256 / lanes" in text
        assert "return mean < 8 ? 4 : mean < 32 ? 16 : 64;" in text
    assert "((int64_t)1 << 22)" in source("sgl_rows.h") and sc.CAP_STREAM == 1 << 22
    agg = source("sgl_aggregate.hip")
    assert f"constexpr int kW1dBlocks = {sc.CAP_W1D};" in agg
    assert "n_edges < 256 * 1024 ? (n_edges + 255) / 256 : 1024" in source("sgl_edge.hip") and (sc.FILL_FROM, sc.FILL_BLOCKS) == (262144, 1024)
    # every loss launch takes its grid from sgl::loss_grid with the kernel's own cap: two sites in K9, K12 and K14 -- the batches of
    # the register kernels through sgl::loss_batch_grid, which hands them to loss_grid, and the streaming kernel -- and one in K11
    common = source("sgl_common.h")
    assert "return {n_batches, loss_grid(n_batches, cap)};" in common and "const int64_t per_batch = (int64_t)groups * u;" in common
    assert "const int64_t n_batches = (n + per_batch - 1) / per_batch;" in common
    for text in (km, cl, zl):
        assert text.count("sgl::loss_batch_grid(n, 256 / LPR, U, kMaxBlocks)") == 1
        assert text.count("sgl::loss_grid((n + 3) / 4, kMaxBlocks)") == 1
        assert text.count("sgl::loss_grid(") + text.count("sgl::loss_batch_grid(") == 2
    assert el.count("sgl::loss_grid((n_fold + 3) / 4, kMaxFoldBlocks)") == 1 and el.count("sgl::loss_grid(") == 1
    # rows per lane group, as the three files write them
    assert "return vec * ch * 4 <= 64 ? 4 : (vec * ch * 2 <= 64 ? 2 : 1);" in km
    assert "return vec * ch * 8 <= 64 ? 4 : (vec * ch * 4 <= 64 ? 2 : 1);" in cl
    assert [sc.k9_rows_per_group(v, c) for v, c in ((1, 1), (1, 16), (1, 32), (4, 1), (4, 4), (4, 6), (4, 8))] == [4, 4, 2, 4, 4, 2, 2]
    # the chunk counts of the 64-lane instances: one list per family and lane size in sgl_common.h, read by the rule
    # (sgl::slice_instance) and by the dispatch (with_slice_instance) of each entry point; K9's are these
    lists = chunk_lists()
    assert sorted(lists) == ["ClassLoss", "ClusterLoss", "EdgeLoss", "Kmeans"]
    assert lists["Kmeans"] == {4: (2, 3, 4, 6, 8), 1: (2, 4, 8, 16, 32)}
    for vec in (1, 4):                                                        # each list against the tests' own restatement
        assert set(lists["Kmeans"][vec]) == {sc.k9_instance(d, vec)[2] for d in range(1, 2600)} - {0, 1}
        assert set(lists["EdgeLoss"][vec]) == {i[3] for i in elc.compiled_instances() if i[1] == vec} - {0, 1}
        assert set(lists["ClusterLoss"][vec]) == {i[2] for i in clc.compiled_instances() if i[1] == vec} - {0, 1}
        assert lists["ClassLoss"][vec] == zlc.CHUNKS[vec]
    assert all(list(v) == sorted(v) for fam in lists.values() for v in fam.values())   # ascending: the rule takes the first that fits
    for text, family, more in ((km, "Kmeans", ""), (cl, "ClusterLoss", ""), (zl, "ClassLoss", ""), (el, "EdgeLoss", ", 0")):
        assert text.count(f"sgl::slice_instance(") == 1 and f"sgl::{family}Slices::chunks(vec))" in text
        assert text.count(f"with_slice_instance<sgl::{family}Slices{more}>(") == 1 and "with_one_of<" not in text.replace("with_one_of<MODE", "")
        assert "#define" not in text
    rows = source("sgl_rows.h")
    assert "with_chunks<MORE...>(typename Family::Vec4{}, in.ch" in rows and "with_chunks<MORE...>(typename Family::Vec1{}, in.ch" in rows
    assert "return with_one_of<MORE..., Cs...>(ch, f);" in rows


def test_pick_lanes_and_stream_grid():
    assert [sc.pick_lanes(0, 10, n) for n in (0, 79, 80, 319, 320)] == [4, 4, 16, 16, 64]
    assert sc.pick_lanes(16, 10, 10 ** 6) == 16 and sc.pick_lanes(0, 0, 5) == 4 and sc.pick_lanes(0, 10, 10, 400) == 64
    assert sc.stream_grid(1).blocks == 1 and sc.stream_grid(257).blocks == 2 and sc.stream_grid(0).blocks == 1
    assert sc.stream_grid(256 * (1 << 22) + 1).blocks == 1 << 22 and sc.stream_grid(256 * (1 << 22) + 1).rounds_max == 2
    assert sc.stream_grid(10 ** 5, 3).blocks == 3
    # the contract shape [111 059 956, 128] in 16-byte elements strides; so do the loss kernels on it, K14 with 172 classes
    assert sc.stream_grid(111059956 * 32).rounds_max >= 2
    assert sc.k14_grid(172, 4, 111059956).work > sc.CAP_K14 and sc.k14_grid(172, 4, 111059956).per_unit == 16
    # K14's cap needs about 9 GB of logits at the narrowest rows: no test at natural size
    assert min(sc.CAP_K14 * sc.per_batch(sc.k14_instance(c, v)) * c * 4 for c in zlc.WIDTHS for v in (1, 4)) > 1 << 27


class _Matrix:
    """what the expected_instance rules of the *_common.py files read of a tensor: two rows of d floats whose pitch and base allow
    16-byte lanes (vec = 4) or do not (vec = 1)"""

    def __init__(self, d, vec):
        self.shape = (2, d)
        self.pitch = -(-d // 4) * 4 if vec == 4 else (d if d % 4 else d + 1)

    def stride(self, dim):
        return self.pitch if dim == 0 else 1

    def data_ptr(self):
        return 0


def test_library_host_rules_equal_the_restatement(tmp_path):
    """sgl::pick_lpr, sgl::slice_instance over the lists of all four families and sgl::loss_grid (host code), built with g++ into
    tests/native/strided_table.cpp"""
    gxx = shutil.which("g++")
    if gxx is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "strided_table")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "native", "strided_table.cpp"), os.path.join(ROOT, "sgl_amd", "csrc", "sgl_core.cpp"),
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    widths = list(range(1, 2600))
    grids = [(w, cap, key) for cap in (2048, 1 << 20) for key in (0, 1, 3, 2048, 5000) for w in (1, 2, 3, 4, 2047, 2048, 2049, 1 << 21)]
    rules = ("cls", "km", "el", "cl")
    queries = [f"lpr {d} {v}" for v in (1, 4) for d in widths] + [f"{rule} {c} {v}" for rule in rules for v in (1, 4) for c in widths]
    queries += [f"grid {w} {cap} {key}" for w, cap, key in grids] + ["grid 7 2048 0"]
    r = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(queries)
    m = 2 * len(widths)
    assert [g[0] for g in got[:m]] == [sc.pick_lpr(d, v) for v in (1, 4) for d in widths]
    width_vec = [(c, v) for v in (1, 4) for c in widths]
    for (lpr, ch), (c, v) in zip(got[m:2 * m], width_vec):
        assert (64 if ch == 0 else lpr, v, ch) == zlc.instance_for(c, v), (c, v, lpr, ch)
    for (lpr, ch), (d, v) in zip(got[2 * m:3 * m], width_vec):                  # K9
        assert (64 if ch == 0 else lpr, v, ch) == sc.k9_instance(d, v)[:3], (d, v, lpr, ch)
    for (lpr, ch), (d, v) in zip(got[3 * m:4 * m], width_vec):                  # K11: ch = 0 is an instance of the same kernel
        assert lpr == sc.pick_lpr(d, v) and (lpr == 64 or ch == 1), (d, v, lpr, ch)
        assert (lpr, v, 0, ch) == elc.expected_instance(_Matrix(d, v), "sigmoid"), (d, v, lpr, ch)
    for (lpr, ch), (d, v) in zip(got[4 * m:5 * m], width_vec):                  # K12, both restatements
        assert (64 if ch == 0 else lpr, v, ch) == sc.k12_instance(d, v)[:3], (d, v, lpr, ch)
        assert sc.k12_instance(d, v) == clc.expected_instance(_Matrix(d, v), _Matrix(d, v)), (d, v)
    for (blocks,), (w, cap, key) in zip(got[5 * m:], grids):
        assert blocks == sc.grid(w, 1, cap, key).blocks == min(w, cap, key if key > 0 else cap), (w, cap, key, blocks)


def test_the_tuning_key():
    assert _lib.get_tuning("loss_blocks") == 0 and _lib.get_tuning("agg_blocks") == 0
    try:
        _lib.set_tuning("loss_blocks", 3)
        assert _lib.get_tuning("loss_blocks") == 3
    finally:
        _lib.set_tuning("loss_blocks", 0)
    assert _lib.get_tuning("loss_blocks") == 0
    with pytest.raises(Exception):
        _lib.set_tuning("loss_block", 1)
    with pytest.raises(Exception):
        _lib.get_tuning("loss_block")
    core = source("sgl_core.cpp")
    assert re.search(r'\{"loss_blocks", 0\}', core) and "loss_blocks" in open(os.path.join(ROOT, "include", "sgl_hip.h")).read()


# ---- (a) forced caps at today's shapes ------------------------------------------------------------------------------------------------------
def forced_ok(make, what):
    """make(forced) -> Grid.  Under every forced cap of the case the launch has more work than workgroups and some workgroup walks
    two units or more; one workgroup walks everything at 1, and at one of the others the trip counts are uneven"""
    caps = sc.forced_caps(make(0).work)
    assert caps[:2] == sc.FORCED and len(caps) <= 3
    grids = [make(c) for c in caps]
    for c, g in zip(caps, grids):
        assert g.cap == c and g.blocks == c and g.work > c and g.rounds_max >= 2, (what, c, g)
    assert grids[0].rounds_min == grids[0].rounds_max == grids[0].work
    assert grids[-1].rounds_min == grids[-1].rounds_max - 1, (what, caps, grids[-1])
    return grids


def test_forced_caps_of_a_launch():
    assert sc.forced_caps(10) == (1, 3) and sc.forced_caps(9) == (1, 3, 2) and sc.forced_caps(258) == (1, 3, 4) and sc.forced_caps(60) == (1, 3, 7)


def test_forced_caps_stride_at_todays_shapes():
    for d, k in kc.cases():
        for layout in kc.LAYOUTS:
            forced_ok(lambda f: sc.k9_grid(d, k, sc.vec_of(layout, d, k), kc.N_ROWS, f), ("K9", d, k, layout))
    for d, k in clc.cases():
        for layout in kc.LAYOUTS:
            forced_ok(lambda f: sc.k12_grid(d, k, sc.vec_of(layout, d, k), kc.N_ROWS, f), ("K12", d, k, layout))
    for c in zlc.WIDTHS:
        for vec in (1, 4):
            for g in forced_ok(lambda f: sc.k14_grid(c, vec, zlc.N_ROWS, f), ("K14", c, vec)):
                # the arg-max cases stand in the last 64 rows: a later round under every forced cap
                assert (zlc.N_ROWS - 64) // g.per_unit // g.blocks >= 1, (c, vec, g)
    folds = {(name, mp): len(plan_tables(edges, EDGE_ROWS, mp)[4]) for name, edges in (("edges", EDGES), ("hub", hub_edges())) for mp in (1, 8)}
    assert folds[("hub", 8)] == 1                                             # the hub alone is cut there: one workgroup whatever the key
    for key, n_fold in folds.items():
        if key != ("hub", 8):
            forced_ok(lambda f: sc.fold_grid(n_fold, f), ("K11", key, n_fold))
    # the multi-tile cases restage in every batch, the others once per workgroup
    for cases, tiles in ((kc.cases(), sc.k9_tiles), (clc.cases(), sc.k12_tiles)):
        multi = {(d, k) for d, k in cases if d <= 2048 and tiles(d, k, 4)[1] > 1}
        assert multi >= {(600, 64), (1030, 64), (257, 130)}
        assert all((k * (-(-d // 4) * 4) > sc.TILE_FLOATS) == ((d, k) in multi) for d, k in cases if d <= 2048)


# ---- (b) forced agg_blocks ------------------------------------------------------------------------------------------------------------------
def test_forced_agg_blocks_stride():
    names = {c[0] for c in sc.AGG_CASES}
    assert names == {"reduce16", "reduce_odd", "wsum2d", "wsum2d_dx", "select_bwd", "lincomb", "concat4", "concat_any", "concat1",
                     "bf16_reduce", "bf16_concat"}
    assert {c[4] for c in sc.AGG_CASES if c[0].startswith("reduce")} == {1, 2, 3, 4}
    for case in sc.AGG_CASES:
        n, threads = case[2], sc.agg_threads(case)
        assert n in (77, 1031)
        grids = forced_ok(lambda f: sc.stream_grid(threads, f), case)
        for g in grids:
            assert threads > 4 * 256 * g.cap and g.partial > 0, (case, threads, g)


# ---- (c) natural caps -----------------------------------------------------------------------------------------------------------------------
def decomposed(n, per, cap):
    """n = cap x per + one more batch + a remainder"""
    rest = n - cap * per - per
    return 0 < rest < per


def test_k9_natural_cases():
    want = {(7, 7): (8, 1, 1, 4), (100, 7): (32, 4, 1, 4), (256, 7): (64, 4, 1, 4), (1030, 17): (64, 4, 6, 2), (2500, 3): (64, 4, 0, 1)}
    for d, k, n, layout in sc.K9_NATURAL:
        vec = sc.vec_of(layout, d)
        inst = sc.k9_instance(d, vec)
        assert inst == want[(d, k)], (d, k, inst)
        g = sc.k9_grid(d, k, vec, n)
        ok(g, ("K9", d, k, n))
        assert g.partial > 0 and decomposed(n, g.per_unit, sc.CAP_K9) and g.cap == sc.CAP_K9, (d, k, n, g)
        assert g.rounds_max == 2 and g.rounds_min == 1
        assert 2048 * g.per_unit < n                                           # the slices of the bit comparison are shorter than n
    assert sc.k9_tiles(1030, 17, 4) == (15, 2) and 17 * 1032 > sc.TILE_FLOATS   # two tiles, restaged in every batch
    assert all(sc.k9_tiles(d, k, sc.vec_of(lay, d))[1] == 1 for d, k, _, lay in sc.K9_NATURAL if d not in (1030, 2500))


@pytest.mark.parametrize("d,k,n,layout", sc.K9_NATURAL)
def test_k9_share_of_near_ties(d, k, n, layout):
    """labels are compared except near ties: the share left out, from the float64 reference alone"""
    near = sc.k9_reference(d, k, n)[4]
    print(f"K9 d = {d}, k = {k}, n = {n}: share of near-tie rows {near.mean():.4f}")
    assert near.mean() <= kc.MAX_LEFT_OUT, (d, k, n, float(near.mean()))


def test_k12_natural_cases():
    want = {(100, 7): (32, 4, 1, 4), (1030, 17): (64, 4, 8, 1), (2500, 3): (64, 4, 0, 1)}
    for d, k, n in sc.K12_NATURAL:
        inst = sc.k12_instance(d, 4)
        assert inst == want[(d, k)], (d, k, inst)
        g = sc.k12_grid(d, k, 4, n)
        ok(g, ("K12", d, k, n))
        assert g.partial > 0 and decomposed(n, g.per_unit, sc.CAP_K12) and g.rounds_max == 2 and g.rounds_min == 1
    assert sc.k12_tiles(1030, 17, 4) == (12, 2, 5) and 17 * 1032 > sc.TILE_FLOATS
    assert sc.k12_tiles(100, 7, 4) == (7, 1, 7)
    for vec in (1, 4):                                                        # the restated instance rule is cluster_loss_common's
        assert {sc.k12_instance(d, vec) for d in range(1, 2600)} == {i for i in clc.compiled_instances() if i[1] == vec}


def test_fold_natural_case():
    edges, n = sc.fold_graph()
    deg = np.bincount(edges.ravel(), minlength=n)
    n_fold = int((deg >= 2).sum())                                            # max_piece = 1: every row with two incidences or more is cut
    assert n_fold == sc.FOLD_RING + 1 and (deg[sc.FOLD_RING + 1:] == 0).all()
    g = sc.fold_grid(n_fold)
    assert n_fold > 4 * sc.CAP_FOLD and g.work > g.cap and g.rounds_max == 2 and g.rounds_min == 1 and g.partial > 0, g


def test_csr_natural_cases():
    lanes_seen = {}
    for lanes, n_rows in sc.CSR_NATURAL:
        g = sc.csr_grid(n_rows, lanes)
        ok(g, ("csr", lanes, n_rows))
        assert n_rows > sc.CAP_CSR * (256 // lanes) and g.rounds_max == 2
        lanes_seen[lanes] = lanes_seen.get(lanes, False) or g.partial > 0
        long_row = sc.csr_long_row(n_rows, lanes)
        assert long_row // g.per_unit // g.blocks == g.rounds_max - 1 and 0 < long_row < n_rows - 1       # in the last round
    assert lanes_seen == {64: True, 16: True, 4: True}                        # a partial last group of rows for every G
    assert sc.CAP_CSR * 4 + 1 == 131073
    a = sc.big_csr(5003, 1, long_row=4990)
    b = sc.big_csr(5003, 4, shared_with=a)
    for m in (a, b):
        length = np.diff(m.indptr)
        assert length[0] == 0 and length[-1] == 0 and set(length.tolist()) >= set(range(10))
        rows = np.repeat(np.arange(5003), length)
        keys = rows.astype(np.int64) * 5003 + m.indices
        assert (np.diff(keys) > 0).all() and m.indices.min() >= 0 and m.indices.max() < 5003           # canonical, in range
    assert np.diff(a.indptr)[4990] == sc.CSR_LONG_ROW
    ra = np.repeat(np.arange(5003), np.diff(a.indptr))
    assert 0.05 < (ra == a.indices).mean() < 0.5                              # self loops for drop_self
    ka = ra.astype(np.int64) * 5003 + a.indices
    kb = np.repeat(np.arange(5003), np.diff(b.indptr)).astype(np.int64) * 5003 + b.indices
    common = np.intersect1d(ka, kb).size
    assert 0.1 * len(ka) < common < 0.9 * len(ka)                             # shared and unshared columns for the merge


def test_wsum1d_and_fill_cases():
    (n, d, H, vec), (n2, d2, H2, vec2) = sc.W1D_NATURAL
    assert vec and not vec2 and d % 4 == 0 and d2 % 4 != 0
    assert n * (d // 4) > sc.CAP_W1D * 256
    blocks, per = sc.w1d_vec(n, d)
    assert per > 256 and per % 256 == 0 and blocks <= sc.CAP_W1D and (n * (d // 4)) % per != 0, (blocks, per)
    assert sc.w1d_vec(5000, 100) == (-(-5000 * 25 // 256), 256)                 # the largest shape tested before: one vector per thread
    g = sc.w1d_scalar_grid(n2, d2)
    ok(g, "wsum1d scalar")
    assert g.partial > 0 and n2 * d2 > 2097152 and sc.w1d_scalar_grid(5000, 100).rounds_max == 1
    g = sc.fill_grid(sc.FILL_EDGES)
    ok(g, "edge_fill")
    assert g.blocks == sc.FILL_BLOCKS and g.partial > 0 and sc.fill_grid(sc.FILL_FROM - 1).rounds_max == 1


def test_row_sample():
    for n, per, cap in ((65573, 32, 2048), (8197, 4, 2048), (16395, 8, 2048)):
        rows = sc.row_sample(n, per, cap)
        batches = set((rows // per).tolist())
        assert {0, cap - 1, cap, n // per - 1, n // per} <= batches and len(rows) >= sc.SAMPLE_ROWS
        assert n - 1 in rows and 0 in rows and np.all(np.diff(rows) > 0)
        for b in (0, cap - 1, cap, n // per - 1):
            assert np.isin(np.arange(b * per, (b + 1) * per), rows).all()

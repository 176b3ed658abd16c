"""The case table of the wide-row tests (tests/wide_common.py), checked without a GPU: it holds exactly the header functions that
take a row width, the launch arithmetic restated there agrees with the constants in the sources, no case is BLIND (every width lies
beyond the threshold it is meant to cross), the sampled forms used for the one case that cannot be materialised equal the full
generator and the full oracle at small widths, and every width the library refuses is refused by name, with the documented code
and message, before anything touches a device."""
import importlib
import re

import numpy as np
import pytest

import oracle
import wide_common as wc
from sgl_amd import _lib, synthetic
from spmm_order_common import cut_rule, default_long_row_nnz, dispatch
from stream_common import _DECL, strip_comments


# ---- the table is complete ---------------------------------------------------------------------------------------------------------
def test_the_parser_finds_width_parameters_by_name():
    text = """/* int fake(int64_t d); */
    int sgl_a(const float *d_x, int64_t ldx, int64_t n,
              int64_t d, void *stream);
    int sgl_b(const float *d_x, int64_t n, void *stream);
    int sgl_c(int row_floats, int64_t pad_cols);
    int64_t sgl_d(int n_hops, int64_t n, int64_t k);
    int sgl_e(const int32_t *d_col, const float *d_c, int64_t ldc);"""
    assert wc.width_functions(text) == {"sgl_a": ["d"], "sgl_c": ["row_floats", "pad_cols"], "sgl_d": ["k"]}


def test_the_table_holds_exactly_the_functions_that_take_a_width():
    """the project's "case list proven complete" idiom: dropping a row, or adding an entry point without one, fails here"""
    declared = wc.declared()
    assert len(declared) == 45
    assert not set(wc.EXCLUDED) & set(wc.CASES)
    assert sorted(set(wc.CASES) | set(wc.EXCLUDED)) == sorted(declared)
    assert all(len(reason) > 20 for reason in wc.EXCLUDED.values())
    families = {c.family for c in wc.CASES.values()}
    assert families == {"spmm", "spmm_bf16", "stream", "concat", "bf16_agg", "rowwise", "limits", "rows", "edges", "losses"}
    assert {c.compare for c in wc.CASES.values()} == {"bits", "truth", "limit"}


def test_dropping_a_case_or_adding_a_prototype_is_noticed():
    declared = set(wc.declared())
    for gone in ("sgl_hop_concat_padded_f32", "sgl_synth_features", "sgl_kmeans_assign_f32"):
        assert sorted(set(wc.CASES) - {gone}) != sorted(declared)
    more = wc.header("sgl_hip.h").replace("int sgl_version(void);", "int sgl_version(void);\nint sgl_new_thing_f32(const float *d_x, int64_t n, int64_t d, void *stream);")
    grown = wc.width_functions(more)
    assert "sgl_new_thing_f32" in grown and sorted(set(grown) | set(wc.width_functions(wc.header("sgl_probe.h")))) != sorted(wc.CASES)


def test_every_case_names_the_wrapper_it_goes_through():
    for entry, c in wc.CASES.items():
        assert entry in _lib.PROTOTYPES or entry in _lib.PROBE_PROTOTYPES, entry
        mod, _, attr = c.via.partition(".")
        obj = importlib.import_module("sgl_amd." + mod)
        for part in attr.split("."):
            obj = getattr(obj, part)
        assert callable(obj), c.via
    # the cases that have a wrapper for these arguments use it; device._call (the one call path under every wrapper) for the rest
    assert {c.via.split(".")[0] for c in wc.CASES.values()} == {"device", "_lib"}


# ---- the constants the arithmetic uses are the sources' --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wc.SOURCE_CONSTANTS))
def test_restated_constants_are_the_sources(name):
    assert wc.source_constant(name) == wc.C[name], (name, wc.SOURCE_CONSTANTS[name][0])


def test_the_documented_limits_are_in_the_header_and_in_the_sources():
    text = re.sub(r"\s+", " ", wc.header("sgl_hip.h").replace("\n *", " "))
    assert "may be at most 2^31 - 1 - 4096" in text and wc.C["SGL_MAX_WIDTH"] == 2 ** 31 - 1 - 4096
    assert "is wider than SGL_MAX_WIDTH=2147479551" in text
    assert "d <= 512. Agrees with the per-prefix" in text                              # sgl_nafs_prefix_f32
    assert "n_hops <= 16, d <= 1024, 16-byte aligned rows, else SGL_ERR_UNSUPPORTED" in text   # sgl_hop_colsum_f32
    assert "row_floats % 4 == 0, <= 256" in re.sub(r"\s+", " ", wc.header("sgl_probe.h").replace("\n *", " "))
    for entry, c in wc.CASES.items():
        if c.compare == "limit":
            assert c.widths[1] > c.widths[0] and c.widths[0] in (256, 512, 1024), entry


# ---- no case is blind ------------------------------------------------------------------------------------------------------------
def test_the_widths_cross_what_they_are_meant_to_cross():
    assert wc.W_CAP > wc.C["kConcatRowCap"] and wc.W_ODD > 2 ** 16 and wc.W_VEC > 2 ** 16 and wc.W_BF16 > 2 ** 16 and wc.W_MEGA > 2 ** 20
    assert wc.W_ODD % 2 == 1 and wc.W_CAP % 4 == 0 and wc.W_VEC % 4 == 0 and wc.W_VEC % 8 != 0 and wc.W_BF16 % 8 == 0 and wc.W_MEGA % 4 == 0
    assert wc.NS == (1, 3, 9) and 9 > wc.C["kConcatRows"] and wc.H == 3 and wc.H_MANY > 16
    assert {n for n, _ in wc.SHAPES} == set(wc.NS) and {w for _, w in wc.SHAPES} == set(wc.WIDTHS)
    # every case runs at a width beyond every register layout of its entry point, and in 64-lane groups
    for entry, c in wc.CASES.items():
        if c.compare == "limit":
            continue
        assert all(w in wc.WIDTHS for w in c.widths) and wc.shapes(c.widths), entry
        for w in c.widths:
            for vec in (1, 4):
                assert w > wc.register_width(entry, vec) and wc.pick_lpr(w, vec) == 64, (entry, w)
    # SpMM: more slices than any test has run (3); the reused split-row workspace crosses all of them
    assert wc.spmm_slices(wc.W_VEC, 4) == 65 and wc.spmm_slices(wc.W_CAP, 1) == 17 and wc.spmm_slices(wc.W_BF16, 8) == 33
    # the flat-index kernels: more than 2^16 lane accesses per row at W_ODD (one float per lane), 2^18 at W_MEGA (four)
    assert wc.W_ODD // 1 > 2 ** 16 and wc.W_MEGA // 4 > 2 ** 18 and wc.col_signature_launches(wc.W_MEGA) == 1025
    # the width as a count: k = 4 100 centres of 7 columns are staged in three LDS tiles, in both lane sizes
    assert wc.centre_tiles(wc.K_WIDE, wc.D_NARROW, 4) == 3 and wc.centre_tiles(wc.K_WIDE, wc.D_NARROW, 1) == 2
    assert wc.K_WIDE > wc.C["kConcatRowCap"]


def test_the_spmm_slices_are_the_dispatch_of_the_order_tests():
    """spmm_slices against spmm_order_common.dispatch (itself compared with the library on the CPU by test_spmm_order_cpu.py)"""
    for dtype, d, ld, lane in (("f32", wc.W_VEC, wc.W_VEC, 4), ("f32", wc.W_CAP, wc.W_CAP + 1, 1), ("bf16", wc.W_BF16, wc.W_BF16, 8)):
        sl = dispatch(dtype, d, ld, ld, 0, 0, False, 5.0)
        assert len(sl) == wc.spmm_slices(d, lane) and sl[0][2][0] == lane and sum(dc for _, dc, _ in sl) == d, (dtype, d)
        assert sl[-1][0] + sl[-1][1] == d and sl[-1][1] < sl[0][1]                      # a narrower last slice


def test_every_concat_route_is_taken_where_it_is_legal():
    rt = wc.concat_route
    # beyond kConcatRowCap the whole-row kernel is never legal: concat_lds = 3 falls back to the tile kernel
    for lds, want in ((0, "any"), (1, "lds"), (3, "lds")):
        assert rt(wc.H, wc.W_ODD, 0, True, lds) == want and rt(wc.H, wc.W_ODD, 5, True, lds) == want
    for w in (wc.W_CAP, wc.W_VEC, wc.W_MEGA):
        assert all(rt(wc.H, w, p, True, lds) == "copy4" for lds in (0, 1, 3) for p in (0, 4))
        assert all(rt(wc.H, w, 0, False, lds) == "copy1" for lds in (0, 1, 3))
    assert rt(wc.H_MANY, wc.W_CAP, 0, True) == "copy4" and rt(wc.H_MANY, wc.W_CAP + 1, 0, True) == "lds"
    # below the cap all five exist (the far-offset tests run them): the restatement tells them apart
    assert rt(4, 147, 4, True, 1) == "rows" and rt(4, 1029, 4, True, 1) == "lds" and rt(4, 7, 4, True, 1) == "any"
    assert rt(4, 250, 0, True, 1) == "lds" and rt(4, 250, 0, True, 3) == "rows" and rt(4, 1024, 0, True, 3) == "copy4"
    assert set(wc.CONCAT_KERNELS) == {"copy4", "copy1", "rows", "lds", "any"}


def test_the_2_31_case_reaches_the_64_bit_branch():
    Hh, d, n = wc.HUGE["H"], wc.HUGE["d"], wc.HUGE["n"]
    assert Hh == wc.C["SGL_MAX_HOPS"] and d * Hh >= 2 ** 31 and d % 4 != 0 and d <= wc.C["SGL_MAX_WIDTH"] and n == 1
    assert wc.concat_route(Hh, d, 0, True) == "copy1" and wc.concat_route(Hh, d, 0, True, 3) == "copy1"
    assert wc.concat_flat_accesses(Hh, d, 1) > wc.INT32_MAX                              # `rem` leaves 32 bits: the branch under test
    assert wc.stream_grid_iterations(n * Hh * d) == 3                                    # ... inside a strided launch
    assert Hh * d * 4 + d * 4 < wc.HUGE_NEEDS
    # the row just below still takes a 16-byte kernel, the one a tile below 2^31 the fallback (the margin the launcher keeps)
    assert wc.concat_route(3, 65537, 0, True) == "lds" and wc.concat_route(3, 715827543, 0, True) == "copy1"
    assert wc.concat_route(3, 715827541, 0, True) == "lds" and 3 * 715827541 == wc.INT32_MAX - wc.C["kConcatTile"]


def test_the_graph_has_a_split_row_and_empty_rows():
    for unit in (False, True):
        g = wc.graph(unit)
        deg = np.diff(g.rowptr)
        lr = default_long_row_nnz(len(g.col))
        assert lr == 32 and deg.max() > lr and (deg == 0).sum() == 2 and len(cut_rule(g.rowptr, lr)) == 2
        assert all((np.diff(g.col[g.rowptr[r]:g.rowptr[r + 1]]) > 0).all() for r in range(g.n))
        assert g.n * wc.W_VEC * 4 < 100e6 / 4                                           # a call (X, Y, residual, aggregate) under 100 MB
    p, perm = wc.permuted(wc.graph())
    assert sorted(perm) == list(range(p.n)) and np.array_equal(np.diff(p.rowptr), np.diff(wc.graph().rowptr)[perm])
    x = wc.hops_host(p.n, 9, 1)[0]
    y = oracle.oracle_spmm(p.rowptr, p.col, p.val, x)
    assert np.array_equal(y, oracle.oracle_spmm(*wc.graph()[1:], x)[perm])             # storage row i is row perm[i]


# ---- the sampled forms equal the full ones ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (1, 5, 64, 1000, 70001))
def test_hashed_columns_one_by_one_equal_the_generator(d):
    full = synthetic.hashed_features_numpy(11, [0, 3], d)
    cols = wc.sample_columns(d, min(d, 40), seed=d)
    assert len(set(cols)) == min(d, 40) and cols.min() == 0 and cols.max() == d - 1
    for k, row in enumerate((0, 3)):
        assert np.array_equal(wc.hashed_features_at(11, row, cols), full[k, cols])
    if d > 2 ** 16:
        assert {2 ** 15 - 1, 2 ** 15, 2 ** 16 - 1, 2 ** 16} <= set(cols)                 # both sides of the 16-bit boundary


@pytest.mark.parametrize("n_hops,d", ((1, 7), (3, 5), (5, 64), (17, 33), (64, 3)))
def test_sampled_concat_equals_the_oracle(n_hops, d):
    """the sampled form of the 2^31 case -- all hop pointers name ONE row -- against oracle.agg_concat over the materialised list"""
    row = synthetic.hashed_features_numpy(5, [0], d)
    full = oracle.agg_concat([row] * n_hops, 0, n_hops)
    assert full.shape == (1, n_hops * d)
    pos, hop, src = wc.concat_samples(n_hops, d, lambda h: wc.sample_columns(d, min(d, 4), seed=h))
    assert np.array_equal(full[0, pos], wc.hashed_features_at(5, 0, src))
    assert set(np.arange(n_hops) * d) <= set(pos) and set(np.arange(1, n_hops + 1) * d - 1) <= set(pos)   # first and last of every segment
    assert np.array_equal(pos // d, hop) and np.array_equal(pos % d, src)
    # and with distinct hops: the positions are hstack's
    hops = wc.hops_host(2, d, n_hops, seed=1)
    full = oracle.agg_concat(hops, 0, n_hops)
    assert all(full[1, p] == hops[h][1, c] for p, h, c in zip(pos, hop, src))


# ---- refusals: by name, documented code and message, before any launch -------------------------------------------------------------
# entry point -> (the name its messages carry, the argument the message names, the other arguments a call needs to get that far)
REFUSED_BY_WIDTH = {
    "sgl_hop_reduce_f32": ("sgl_hop_reduce_f32", "d", {}),
    "sgl_hop_wsum2d_f32": ("sgl_hop_wsum2d_f32", "d", {}),
    "sgl_hop_wsum2d_bwd_f32": ("sgl_hop_wsum2d_bwd_f32", "d", {}),
    "sgl_hop_rowdot_f32": ("sgl_hop_rowdot_f32", "d", {}),
    "sgl_hop_wsum1d_bwd_f32": ("sgl_hop_wsum1d_bwd_f32", "d", {}),
    "sgl_hop_select_bwd_f32": ("sgl_hop_select_bwd_f32", "d", {"op": 2}),
    "sgl_hop_lincomb_f32": ("sgl_hop_lincomb_f32", "d", {}),
    "sgl_hop_concat_f32": ("sgl_hop_concat_f32", "d", {}),
    "sgl_hop_concat_padded_f32": ("sgl_hop_concat_f32", "d", {}),
    "sgl_nafs_f32": ("sgl_nafs_f32", "d", {}),
    "sgl_nafs_padded_f32": ("sgl_nafs_f32", "d", {}),
    "sgl_gather_rows_f32": ("sgl_gather_rows_f32", "d + pad_cols", {}),
    "sgl_gather_rows_padded_f32": ("sgl_gather_rows_padded_f32", "d + pad_cols", {}),
    "sgl_gather_hops_padded_f32": ("sgl_gather_hops_padded_f32", "d + pad_cols", {}),
    "sgl_scatter_rows_f32": ("sgl_scatter_rows_f32", "d + pad_cols", {}),
    "sgl_col_signature_f32": ("sgl_col_signature_f32", "d", {}),
    "sgl_edge_dot_f32": ("sgl_edge_dot_f32", "d", {}),
    "sgl_edge_loss_grad_f32": ("sgl_edge_loss_grad_f32", "d", {}),
    "sgl_kmeans_assign_f32": ("sgl_kmeans_assign_f32", "d", {"k": 1}),
    "sgl_cluster_loss_grad_f32": ("sgl_cluster_loss_grad_f32", "d", {"k": 1}),
    "sgl_hop_reduce_bf16_f32": ("sgl_hop_reduce_bf16_f32", "d", {}),
    "sgl_hop_concat_bf16": ("sgl_hop_concat_bf16", "d", {}),
    "sgl_hop_concat_bf16_f32": ("sgl_hop_concat_bf16_f32", "d", {}),
    "sgl_gather_rows_bf16_f32": ("sgl_gather_rows_bf16_f32", "d + pad_cols", {}),
    "sgl_gather_hops_bf16_f32": ("sgl_gather_hops_bf16_f32", "d + pad_cols", {}),
    "sgl_synth_features": ("sgl_synth_features", "d", {"ld": 2 ** 31}),
}
# the entry points whose width check needs a handle (the SpMM family) are refused in test_gpu_wide_rows.py; the "limit" cases and the
# class loss document narrower limits of their own
NEEDS_A_HANDLE = {e for e, c in wc.CASES.items() if c.family in ("spmm", "spmm_bf16")}


def parameters(entry):
    text = strip_comments(wc.header("sgl_hip.h") + wc.header("sgl_probe.h"))
    for m in _DECL.finditer(text):
        if m.group(1) == entry:
            return [(p.strip(), re.findall(r"\w+", p)[-1]) for p in m.group(2).split(",")]
    raise KeyError(entry)


def call_with(entry, **values):
    """the entry point on NULL pointers and zero sizes (no rows, one hop), with the named arguments set: every refusal pinned here
    happens before a pointer is looked at"""
    probe = entry in _lib.PROBE_PROTOTYPES
    fn = getattr(_lib.probe_lib() if probe else _lib.lib(), entry)
    args = []
    for decl, name in parameters(entry):
        if name in values:
            args.append(values[name])
        elif "*" in decl:
            args.append(None)
        elif decl.startswith("float"):
            args.append(0.0)
        else:
            args.append(1 if name in ("n_hops", "n_in", "n_out") else 0)
    rc = fn(*args)
    return rc, (_lib.probe_lib().sgl_probe_last_error().decode() if probe else _lib.last_error())


def test_every_entry_point_is_refused_by_width_or_says_why_not():
    limit = {e for e, c in wc.CASES.items() if c.compare == "limit"}
    assert set(REFUSED_BY_WIDTH) | NEEDS_A_HANDLE | limit | {"sgl_class_loss_grad_f32"} == set(wc.CASES)


@pytest.mark.parametrize("entry", sorted(REFUSED_BY_WIDTH))
def test_a_row_wider_than_the_limit_is_refused_by_name(entry):
    who, what, more = REFUSED_BY_WIDTH[entry]
    top = wc.C["SGL_MAX_WIDTH"]
    rc, msg = call_with(entry, d=top + 1, **more)
    assert rc == _lib.SGL_ERR_UNSUPPORTED == 1003, (rc, msg)
    assert msg == f"{who}: {what}={top + 1} is wider than SGL_MAX_WIDTH={top}", msg
    rc, msg = call_with(entry, d=top, **more)                                            # the limit itself is a width like any other
    assert "wider than" not in msg or rc == 0, msg
    rc, msg = call_with(entry, d=2 ** 31 - 1, **more)                                    # 2^31 - 1 and beyond stay "bad sizes"
    assert rc == 1001 and "wider than" not in msg and who in msg, (rc, msg)
    if "pad_cols" in [n for _, n in parameters(entry)] and what == "d + pad_cols":       # the pad counts
        rc, msg = call_with(entry, d=top - 3, pad_cols=4, **more)
        assert rc == 1003 and msg == f"{who}: {what}={top + 1} is wider than SGL_MAX_WIDTH={top}", msg


def test_the_class_loss_keeps_its_own_limit():
    rc, msg = call_with("sgl_class_loss_grad_f32", c=2 ** 30 + 1)
    assert rc == 1001 and msg == "sgl_class_loss_grad_f32: bad sizes (n >= 0, 1 <= c <= 2^30)", msg
    assert 2 ** wc.C["class_loss_max_c_log2"] < wc.C["SGL_MAX_WIDTH"]


def test_the_narrow_limits_are_refused_without_a_launch():
    """sgl_nafs_prefix_f32 (512), sgl_probe_gather_f32 (256 floats) and the scratch size of sgl_hop_colsum_f32 (1 024) answer from
    the host alone; the others of the "limit" cases need device pointers to get as far and are pinned in test_gpu_wide_rows.py"""
    rc, msg = call_with("sgl_nafs_prefix_f32", d=513)
    assert rc == 1001 and msg == "sgl_nafs_prefix_f32: rows of up to 512 floats (d=513)", msg
    rc, msg = call_with("sgl_probe_gather_f32", row_floats=260, ld=260, in_flight=8)
    assert rc == 1001 and msg.startswith("sgl_probe_gather_f32:"), msg
    scratch = _lib.lib().sgl_hop_colsum_scratch
    assert scratch(3, 9, 1024) > 0 and scratch(3, 9, 1025) == 0


# ---- the streaming centre kernels' lane order, restated: one running sum against blocks of 64 chunks ----------------------------------
def lane_order_sum(diff, block):
    """sum of diff^2 in the order of kmeans_assign_stream_kernel / cluster_loss_stream_kernel with 16-byte lanes, in numpy float32
    (rounded product then add where the kernel has an fma: the same order, not the same bits): lane l takes the vectors l, l + 64, ...;
    two accumulators per lane (elements 0, 2 and 1, 3 of a vector); `block` chunks are summed from zero and added to the lane's
    total in order; the 64 lanes are folded pairwise"""
    d = len(diff)
    v = np.zeros((d + 255) // 256 * 256, np.float32)
    v[:d] = diff
    v = v.reshape(-1, 64, 4)
    tot = np.zeros((2, 64), np.float32)
    for b in range(0, len(v), block):
        a = np.zeros((2, 64), np.float32)
        for i in range(b, min(b + block, len(v))):
            a[0] = a[0] + v[i, :, 0] * v[i, :, 0]
            a[1] = a[1] + v[i, :, 1] * v[i, :, 1]
            a[0] = a[0] + v[i, :, 2] * v[i, :, 2]
            a[1] = a[1] + v[i, :, 3] * v[i, :, 3]
        tot = tot + a
    s = tot[0] + tot[1]
    while len(s) > 1:
        s = s[0::2] + s[1::2]
    return float(s[0])


def test_one_running_sum_per_lane_loses_what_blocks_of_64_chunks_keep():
    """What test_gpu_wide_rows.py measured on the MI355X at d = 1 048 580 (cluster-loss dX 4.5e-6 off where numpy's float32 is
    3.6e-7), reproduced from the lane order alone: with one running sum per lane the squared distance of two k-means test rows comes out
    more than 5e-6 low -- their columns 0 .. 7, the first chunk of lanes 0 and 1, carry four fifths of the energy, and every later term
    of those lanes is rounded against that sum -- while blocks of kStreamBlock = 64 chunks stay within 5e-7, like numpy's pairwise sum.
    A row of at most 64 chunks per lane is one block: the same additions, the same bits."""
    import kmeans_common as kc
    assert re.search(r"constexpr int kStreamBlock = 64;", open(wc.ROOT + "/sgl_amd/csrc/sgl_centres.h").read())
    x = kc.host_x(wc.W_MEGA, n=7)
    diff = x[0] - x[1]
    t = float((diff.astype(np.float64) ** 2).sum())
    one, blocked, pairwise = lane_order_sum(diff, 1 << 30), lane_order_sum(diff, 64), float((diff * diff).sum(dtype=np.float32))
    assert (one - t) / t < -5e-6 and abs(blocked - t) / t < 5e-7 and abs(pairwise - t) / t < 1e-6, ((one - t) / t, (blocked - t) / t, (pairwise - t) / t)
    short = diff[:16384]
    assert lane_order_sum(short, 64) == lane_order_sum(short, 1 << 30)

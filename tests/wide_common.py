"""Shared by test_wide_cpu.py and test_gpu_wide_rows.py (importable without a GPU): the case table of the wide-row tests, the launch
arithmetic that decides which kernel a width reaches, restated ONCE here and compared with the constants in the sources, and the
inputs.

Every entry point of include/sgl_hip.h and include/sgl_probe.h that takes a row width (a parameter named d, dz, c, k, row_floats or
pad_cols) has a row in CASES or a reason in EXCLUDED; test_wide_cpu.py proves that by parsing the headers.  A row says which family
of test_gpu_wide_rows.py runs the entry point, how its result is compared, and at which widths; the GPU module records every
(entry point, width, layout) it ran and its last test compares that record with this table.

The widths are the smallest that cross what the code dispatches on: W_CAP = 4 100 is beyond kConcatRowCap (and beyond every register
layout: 512 floats for the row-register aggregators, 1 024 for the class loss, 2 048 for k-means, the cluster loss and the edge loss),
W_ODD = 65 537 is beyond 2^16 and odd (one float per lane everywhere), W_VEC = 65 540 the same with 16-byte lanes (65 SpMM column
slices of 1 024), W_BF16 = 65 544 a multiple of 8 (bfloat16 lanes of 8 elements: 33 slices of 2 048), W_MEGA = 1 048 580 is beyond
2^20.  The one case beyond 2^31 is the float32 concat with H = 64 hops of d = 33 554 433 columns: H d = 2^31 + 64, d % 4 = 1.

No reference is written here: the GPU module imports the oracle each entry point's own test uses.  What IS here is the sampled form
of the two references that the 2^31 case cannot materialise (an 8.6 GB row): hashed input columns recomputed one by one
(hashed_features_at) and the places of a concatenated row where they must appear (concat_samples); test_wide_cpu.py proves both equal
to the full generator / the full oracle at small widths."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from stream_common import _DECL, strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W_CAP, W_ODD, W_VEC, W_BF16, W_MEGA = 4100, 65537, 65540, 65544, 1048580
WIDTHS = (W_CAP, W_ODD, W_VEC, W_BF16, W_MEGA)
NS = (1, 3, 9)                          # 9 = one full row block of the concat tile kernel (8 rows) and a remainder
H, H_MANY = 3, 17                       # 17 hops (beyond the 16 of every register layout) at the smallest width only
# (n, W) pairs every family draws from: all three row counts at the two widths where a row block matters, one or two elsewhere
SHAPES = ((1, W_CAP), (3, W_CAP), (9, W_CAP), (9, W_ODD), (1, W_VEC), (3, W_VEC), (9, W_VEC), (3, W_BF16), (1, W_MEGA), (3, W_MEGA))
HUGE = {"H": 64, "d": 33_554_433, "n": 1}        # float32 concat: H d = 2^31 + 64 columns, an 8.6 GB output row
HUGE_NEEDS = 10 << 30                   # free device memory the 2^31 case asks for
SENTINEL32 = 0x7FC07FC0                 # what outputs are pre-filled with: a NaN no kernel produces and no input holds (far_common.FILL32)
GUARD_ROWS = 2                          # sentinel rows after the last row of every output
WIDTH_PARAMS = ("d", "dz", "c", "k", "row_floats", "pad_cols")
INT32_MAX = 2 ** 31 - 1


def shapes(widths):
    return [(n, w) for n, w in SHAPES if w in widths]


# ---- the table ------------------------------------------------------------------------------------------------------------------
# compare: "bits"    bit for bit with the reference of the entry point's own small test
#          "truth"   oracle.truth_report(HIP, numpy float32 evaluation, float64 truth): err <= max(2 err(ref32), 16 ulp)
#          "limit"   the header documents a narrower width limit: right at the limit, refused one past it, no launch
# via: what test_gpu_wide_rows.py really calls -- the device.py wrapper where it can write into the caller's (sentinel-filled, guarded)
#      buffer; device._call, the one call path under every wrapper, where the wrapper allocates its own output (hop_reduce, hop_concat,
#      nafs_aggregate, ...) or takes other arguments; probe_lib() for the generator (synthetic.hashed_features_torch allocates)
Case = namedtuple("Case", "family compare widths via")
ALL4 = (W_CAP, W_ODD, W_VEC, W_MEGA)
SPMM_W = (W_CAP, W_VEC)                 # W_CAP on an odd pitch (one float per lane, 17 slices of 256), W_VEC (65 slices of 1 024)

CASES = {
    # SpMM: the suite's strict / fast references (oracle_spmm, oracle_spmm_slots), default and strict handles, with and without a row map
    "sgl_spmm_f32": Case("spmm", "bits", SPMM_W, "device.DeviceCSR.spmm"),
    "sgl_spmm_axpb_clamp_f32": Case("spmm", "bits", SPMM_W, "device.DeviceCSR.spmm_axpb_clamp"),
    "sgl_spmm_acc_f32": Case("spmm", "bits", SPMM_W, "device._call"),
    "sgl_spmm_multi_f32": Case("spmm", "bits", SPMM_W, "device.DeviceCSR.spmm_multi"),
    "sgl_spmm_chain_f32": Case("spmm", "bits", SPMM_W, "device.DeviceCSR.spmm_chain"),
    "sgl_chain_graph_create": Case("spmm", "bits", SPMM_W, "device.DeviceCSR.capture_chain"),
    "sgl_spmm_bf16": Case("spmm_bf16", "bits", (W_BF16,), "device.DeviceCSR.spmm"),
    "sgl_spmm_chain_bf16": Case("spmm_bf16", "bits", (W_BF16,), "device.DeviceCSR.spmm_chain"),
    "sgl_spmm_acc_bf16": Case("spmm_bf16", "bits", (W_BF16,), "device.DeviceCSR.spmm_acc"),
    # streaming aggregators: one flat index divided by the width
    "sgl_hop_reduce_f32": Case("stream", "bits", ALL4, "device._call"),
    "sgl_hop_wsum2d_f32": Case("stream", "truth", ALL4, "device._call"),
    "sgl_hop_wsum2d_bwd_f32": Case("stream", "truth", ALL4, "device._call"),
    "sgl_hop_wsum1d_bwd_f32": Case("stream", "truth", ALL4, "device._call"),
    "sgl_hop_select_bwd_f32": Case("stream", "bits", ALL4, "device._call"),
    "sgl_hop_lincomb_f32": Case("stream", "bits", ALL4, "device._call"),
    "sgl_hop_concat_f32": Case("concat", "bits", ALL4, "device._call"),
    "sgl_hop_concat_padded_f32": Case("concat", "bits", ALL4, "device._call"),
    "sgl_hop_reduce_bf16_f32": Case("bf16_agg", "bits", (W_CAP, W_ODD, W_BF16), "device._call"),
    "sgl_hop_concat_bf16": Case("bf16_agg", "bits", (W_CAP, W_ODD, W_BF16), "device._call"),
    "sgl_hop_concat_bf16_f32": Case("bf16_agg", "bits", (W_CAP, W_ODD, W_BF16), "device._call"),
    # row-wise aggregators beyond their register layouts (the two-pass NAFS, the general row-dot)
    "sgl_nafs_f32": Case("rowwise", "truth", ALL4, "device._call"),
    "sgl_nafs_padded_f32": Case("rowwise", "truth", ALL4, "device._call"),
    "sgl_hop_rowdot_f32": Case("rowwise", "truth", ALL4, "device._call"),
    # ... and the ones whose header documents a limit
    "sgl_nafs_prefix_f32": Case("limits", "limit", (512, 513), "device._call"),
    "sgl_nafs_bf16_f32": Case("limits", "limit", (512, 513), "device._call"),
    "sgl_hop_gate_f32": Case("limits", "limit", (512, 513), "device._call"),
    "sgl_hop_gate_padded_f32": Case("limits", "limit", (512, 513), "device._call"),
    "sgl_hop_recursive_f32": Case("limits", "limit", (512, 513), "device._call"),
    "sgl_hop_rowdot2_f32": Case("limits", "limit", (512, 513), "device._call"),
    "sgl_hop_colsum_f32": Case("limits", "limit", (1024, 1025), "device._call"),
    "sgl_hop_colsum_scratch": Case("limits", "limit", (1024, 1025), "_lib.lib"),
    "sgl_probe_gather_f32": Case("limits", "limit", (256, 260), "_lib.probe_lib"),
    # rows and edges
    "sgl_gather_rows_f32": Case("rows", "bits", ALL4, "device._call"),
    "sgl_gather_rows_padded_f32": Case("rows", "bits", ALL4, "device.gather_rows"),
    "sgl_gather_hops_padded_f32": Case("rows", "bits", ALL4, "device._call"),
    "sgl_scatter_rows_f32": Case("rows", "bits", ALL4, "device.scatter_rows"),
    "sgl_gather_rows_bf16_f32": Case("rows", "bits", (W_CAP, W_ODD, W_BF16), "device._call"),
    "sgl_gather_hops_bf16_f32": Case("rows", "bits", (W_CAP, W_ODD, W_BF16), "device._call"),
    "sgl_col_signature_f32": Case("rows", "bits", ALL4, "device.column_signature"),
    "sgl_synth_features": Case("rows", "bits", ALL4, "_lib.probe_lib"),
    "sgl_edge_dot_f32": Case("edges", "truth", ALL4, "device.edge_dot"),
    "sgl_edge_loss_grad_f32": Case("edges", "truth", ALL4, "device.edge_loss_grad"),
    # losses and k-means: the width as a row (d, c) and as a count (k)
    "sgl_class_loss_grad_f32": Case("losses", "truth", ALL4, "device.class_loss_grad"),
    "sgl_cluster_loss_grad_f32": Case("losses", "truth", ALL4, "device.cluster_loss_grad"),
    "sgl_kmeans_assign_f32": Case("losses", "truth", ALL4, "device.kmeans_assign"),
}
EXCLUDED = {}                           # every width-taking entry point has a case
K_WIDE, D_NARROW = 4100, 7              # the centre kernels with the width as a COUNT: k = 4 100 centres of 7 columns
KS = (1, 3)                             # centres at d = W


def width_functions(header_text):
    """{function: [width parameters]} of the functions a header declares with a parameter named like a width"""
    out = {}
    for m in _DECL.finditer(strip_comments(header_text)):
        names = [re.findall(r"\w+", p)[-1] for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
        hit = [p for p in names if p in WIDTH_PARAMS]
        if hit:
            out[m.group(1)] = hit
    return out


def header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def declared():
    out = width_functions(header("sgl_hip.h"))
    out.update(width_functions(header("sgl_probe.h")))
    return out


# ---- constants in the sources --------------------------------------------------------------------------------------------------
# name -> (file under sgl_amd/csrc or include, regular expression with one group, the value the arithmetic below uses)
SOURCE_CONSTANTS = {
    "kConcatRowCap": ("sgl_amd/csrc/sgl_aggregate.hip", r"constexpr int kConcatRowCap = (\d+);", 4096),
    "kConcatTile": ("sgl_amd/csrc/sgl_aggregate.hip", r"constexpr int kConcatTile = (\d+);", 1024),
    "kConcatRows": ("sgl_amd/csrc/sgl_aggregate.hip", r"constexpr int kConcatRows = (\d+);", 8),
    "kConcatLds": ("sgl_amd/csrc/sgl_aggregate.hip", r"constexpr int kConcatLds = (\d+);", 8192),
    "kW1dBlocks": ("sgl_amd/csrc/sgl_aggregate.hip", r"constexpr int kW1dBlocks = (\d+);", 8192),
    "stream_grid_cap_log2": ("sgl_amd/csrc/sgl_rows.h", r"\(\(int64_t\)1 << (\d+)\);\s*\n\s*if \(blocks > cap\)", 22),
    "kTileFloats": ("sgl_amd/csrc/sgl_centres.h", r"constexpr int kTileFloats = (\d+);", 16384),
    "spmm_lanes_f32": ("sgl_amd/csrc/sgl_spmm.hip", r"const int64_t max_cols = 64 \* (\d+) \* vec;", 4),
    "spmm_lanes_bf16": ("sgl_amd/csrc/sgl_spmm_bf16.hip", r"const int64_t max_cols = 64 \* (\d+) \* bv;", 4),
    "class_loss_vec4_chunks": ("sgl_amd/csrc/sgl_common.h", r"using ClassLossSlices = SliceFamily<Chunks<[\d, ]*?(\d+)>, Chunks<2, 4, 8, 16>>;", 4),
    "class_loss_max_c_log2": ("sgl_amd/csrc/sgl_class_loss.hip", r"c <= \(\(int64_t\)1 << (\d+)\)", 30),
    "SGL_MAX_WIDTH": ("include/sgl_hip.h", r"#define SGL_MAX_WIDTH (\d+)", INT32_MAX - 4096),
    "SGL_MAX_HOPS": ("include/sgl_hip.h", r"#define SGL_MAX_HOPS (\d+)", 64),
}
C = {k: v[2] for k, v in SOURCE_CONSTANTS.items()}


def source_constant(name):
    path, pattern, _ = SOURCE_CONSTANTS[name]
    with open(os.path.join(ROOT, path)) as f:
        m = re.search(pattern, f.read())
    return None if m is None else int(m.group(1))


# ---- launch arithmetic -----------------------------------------------------------------------------------------------------------
def spmm_slices(d, lane):
    """column slices of one SpMM call whose lanes hold `lane` elements (spmm_impl of both files): 64 lanes x 4 chunks x lane"""
    cols = 64 * C["spmm_lanes_f32"] * lane
    return (d + cols - 1) // cols


def concat_route(n_hops, d, pad, aligned, concat_lds=1):
    """the kernel sgl_hop_concat_padded_f32 launches (its branches in their order).  aligned: output and hop rows are 16-byte
    aligned on pitches that are multiples of 4 floats.  "copy4" / "copy1": hop_concat_kernel<4> / <1>, "rows": hop_concat_rows_kernel
    (whole rows in LDS, up to kConcatRowCap floats), "lds": hop_concat_lds_kernel (tiles), "any": hop_concat_any_kernel"""
    width = n_hops * d
    if aligned and d % 4 == 0:
        return "copy4"
    out16 = aligned and width + pad <= INT32_MAX - C["kConcatTile"]
    common = out16 and d >= 4
    wcols = width + pad
    tiles = (wcols + C["kConcatTile"] - 1) // C["kConcatTile"]
    if common and width >= 256 and wcols <= C["kConcatRowCap"] and (concat_lds == 3 or (concat_lds == 1 and 100 * wcols < 85 * C["kConcatTile"] * tiles)):
        return "rows"
    if common and width >= 256 and concat_lds != 0:
        return "lds"
    return "any" if common else "copy1"


CONCAT_KERNELS = {"copy4": ("hop_concat_kernel", 4), "copy1": ("hop_concat_kernel", 1), "rows": ("hop_concat_rows_kernel", None),
                  "lds": ("hop_concat_lds_kernel", None), "any": ("hop_concat_any_kernel", None)}


def concat_flat_accesses(n_hops, d, vec):
    """lane accesses per row of hop_concat_kernel<vec>: what its flat index is divided by and what `rem` runs up to"""
    return (d // vec) * n_hops


def pick_lpr(d, vec):
    from agg_rows_common import pick_lpr as rule
    return rule(d, vec)


def register_width(entry, vec):
    """the widest row the register-resident kernel of an entry point holds; beyond it the entry point streams (or runs its
    general kernel, or refuses: the "limit" cases)"""
    if entry == "sgl_class_loss_grad_f32":
        return 64 * vec * (C["class_loss_vec4_chunks"] if vec == 4 else 16)              # 1 024 either way
    if entry in ("sgl_kmeans_assign_f32", "sgl_cluster_loss_grad_f32", "sgl_edge_loss_grad_f32"):
        return 64 * vec * (8 if vec == 4 else 32)                                        # 2 048 either way
    return 512                                                                           # row_instance: 64 lanes x 2 chunks x 4 floats


def centre_tiles(k, d, vec):
    """LDS tiles the k centres of d columns are staged in (launch_assign / launch_loss: pitch d rounded up to the lane size)"""
    dp = (d + vec - 1) // vec * vec
    per = C["kTileFloats"] // dp
    return (k + per - 1) // per


def stream_grid_iterations(total_threads):
    """grid-stride iterations of a stream_grid launch (256 threads per block, at most 2^22 blocks)"""
    cap = (1 << C["stream_grid_cap_log2"]) * 256
    return (total_threads + cap - 1) // cap


def col_signature_launches(d):
    return ((d + 3) // 4 * 4 + 1023) // 1024


# ---- inputs --------------------------------------------------------------------------------------------------------------------
_HOPS = {}


def hops_host(n, d, n_hops, seed=0):
    """[hash_matrix scaled by (1 - 0.04 h)]: distinct from row to row, column to column and hop to hop; built once per shape"""
    from inputs import hash_matrix
    have = _HOPS.setdefault((n, d, seed), [])
    for h in range(len(have), n_hops):
        have.append(np.ascontiguousarray((hash_matrix(n, d, seed=9000 + 100 * seed + 31 * (d % 9973) + h) * np.float32(1.0 - 0.04 * h)).astype(np.float32)))
    if len(_HOPS) > 6:
        _HOPS.pop(next(iter(_HOPS)))
    return have[:n_hops]


def hashed_features_at(seed, row, cols):
    """column `cols` of row `row` of the seeded feature matrix (sgl_synth_features, synthetic.hashed_features_numpy), one by one:
    the generator is keyed by (seed, row, column), so a column costs nothing but itself"""
    from sgl_amd import synthetic
    h = synthetic._hash4(seed, 3, np.full(len(cols), row, dtype=np.int64), np.asarray(cols, dtype=np.int64))
    q = (h >> np.uint64(40)).astype(np.int64) - (1 << 23)
    return (q.astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)


def sample_columns(d, m, seed=0):
    """m distinct columns of [0, d): the first, the last, the two sides of every 2^k boundary below d from 2^15 on (where a narrowed
    column index wraps), then seeded draws"""
    cols = {0, d - 1}
    for k in range(15, 32):
        for c in ((1 << k) - 1, 1 << k):
            if 0 <= c < d:
                cols.add(c)
    rng = np.random.default_rng(1000 + seed)
    while len(cols) < m:
        cols.add(int(rng.integers(0, d)))
    return np.array(sorted(cols), dtype=np.int64)


def concat_samples(n_hops, d, cols_of):
    """(positions int64, hop int64, source column int64): the places of a concatenated row that hold column c of hop h, for the
    columns cols_of(h) of every hop -- out[h d + c] = X_h[c] (ConcatMessageOp: torch.hstack)"""
    pos, hop, src = [], [], []
    for h in range(n_hops):
        c = np.asarray(cols_of(h), dtype=np.int64)
        pos.append(h * d + c)
        hop.append(np.full(len(c), h, dtype=np.int64))
        src.append(c)
    return np.concatenate(pos), np.concatenate(hop), np.concatenate(src)


# ---- the SpMM graph --------------------------------------------------------------------------------------------------------------
Graph = namedtuple("Graph", "n rowptr col val")


@functools.lru_cache(maxsize=None)
def graph(unit_rows=False):
    """A canonical CSR [61, 61], not symmetric: a ring, two seeded neighbours per row, row 5 tied to 45 nodes -- above the
    long_row_nnz of a matrix this small (32), so the default handle cuts it in two pieces and the fix-up kernel runs -- and two empty
    rows.  61 rows because the operand is [n, 65 540]: the suite's other split-row graphs have 1 031 to 1 500 rows, a quarter of a
    gigabyte per matrix at that width.  Values are multiples of 1 / 16 (unit_rows: divided by the row's length, for the bfloat16
    chain)."""
    import scipy.sparse as sp
    n = 61
    rng = np.random.default_rng(61)
    i = np.arange(n)
    r = np.concatenate((i, np.repeat(i, 2), np.full(45, 5)))
    c = np.concatenate(((i + 1) % n, rng.integers(0, n, 2 * n), rng.choice(n, 45, replace=False)))
    keep = ~np.isin(r, (17, 40))
    a = sp.coo_matrix((np.ones(int(keep.sum()), dtype=np.float32), (r[keep], c[keep])), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    rows = np.repeat(i, np.diff(a.indptr))
    val = ((1 + (rows * 7 + a.indices * 3) % 15) / 16.0 * np.where((rows + a.indices) % 3 == 0, -1, 1)).astype(np.float32)
    if unit_rows:
        val = (val / np.maximum(np.diff(a.indptr), 1)[rows]).astype(np.float32)
    return Graph(n, a.indptr.astype(np.int64), a.indices.astype(np.int32), val)


def permuted(g, seed=3):
    """(graph with its rows stored in the order perm, perm): what a handle with a row map wraps (storage row i = row perm[i])"""
    perm = np.random.default_rng(seed).permutation(g.n)
    deg = np.diff(g.rowptr)
    ptr = np.concatenate([[0], np.cumsum(deg[perm])]).astype(np.int64)
    take = np.concatenate([np.arange(g.rowptr[r], g.rowptr[r + 1]) for r in perm]).astype(np.int64)
    return Graph(g.n, ptr, g.col[take], g.val[take]), perm.astype(np.int32)

"""Shared by test_strided_cpu.py and test_gpu_strided_grids.py (importable without a GPU): the launch arithmetic of every entry point
whose launcher caps its grid and lets the workgroups stride over the work beyond the cap, restated from the launchers, the case lists
of the strided tests with what that arithmetic says about each case, input builders at arbitrary n, and the row sample.

A `Grid` is what a launch looks like from the loop `for (b = blockIdx.x; b < work; b += gridDim.x)`: `work` units (batches of rows,
blocks of elements), `blocks` workgroups, each of which walks `rounds_max` or `rounds_min` units.  A case tests a strided path when
work > cap, rounds_max >= 2, and -- unless one workgroup does everything -- rounds_min == rounds_max - 1 (the trip counts are uneven);
the last unit is partial when the item count is no multiple of the items per unit.

Caps, from the sources: K9 / K12 2048 workgroups (sgl_kmeans.hip, sgl_cluster_loss.hip), K14 2^20 (sgl_class_loss.hip), the K11 fold
2048 (sgl_edge_loss.hip), K13 / K15 32768 (sgl_csr_select.hip, sgl_csr_merge.hip), stream_grid 2^22 (sgl_rows.h), the wsum1d
backward 8192 (sgl_aggregate.hip), edge_fill 1024 from 262144 edges on (sgl_edge.hip).  The tuning key loss_blocks (K9, K11's fold,
K12, K14) and agg_blocks (stream_grid) lower a cap when > 0."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import class_loss_common as zlc
import cluster_loss_common as clc
import kmeans_common as kc
from edge_scores_common import pick_lpr

TILE_FLOATS = 16384                                # kTileFloats: 64 KiB of centres per LDS tile
K12_STEP = 4                                       # kStep of sgl_cluster_loss.hip: a tile holds whole steps
CAP_K9 = CAP_K12 = CAP_FOLD = 2048
CAP_K14 = 1 << 20
CAP_CSR = 32768
CAP_STREAM = 1 << 22
CAP_W1D = 8192
FILL_BLOCKS, FILL_FROM = 1024, 256 * 1024
FORCED = (1, 3)                                    # the forced caps: one workgroup walks everything; uneven trip counts
SAMPLE_ROWS = 2000

Grid = namedtuple("Grid", "items per_unit work cap blocks rounds_max rounds_min partial")


def grid(items, per_unit, cap, forced=0):
    """the Grid of `items` items in units of `per_unit` under `cap` workgroups (forced > 0: the tuning key lowers the cap)"""
    if forced > 0 and forced < cap:
        cap = forced
    work = -(-items // per_unit)
    blocks = max(min(work, cap), 1)
    return Grid(items, per_unit, work, cap, blocks, -(-work // blocks), work // blocks, items % per_unit)


def forced_caps(work):
    """the forced caps of a launch of `work` units: 1 and 3, and where 3 workgroups would all walk the same number of units (work a
    multiple of 3) the smallest of 2, 4, 5, 7 that leaves them uneven"""
    if work % 3:
        return FORCED
    return FORCED + (next(c for c in (2, 4, 5, 7) if work % c and work > c),)


def strides(g):
    """the three properties of the module docstring"""
    return g.work > g.cap and g.rounds_max >= 2 and (g.blocks == 1 or g.rounds_min == g.rounds_max - 1) and g.partial > 0


# ---- K9 kmeans_assign_kernel --------------------------------------------------------------------------------------------------------------
def k9_rows_per_group(vec, ch):
    return 4 if vec * ch * 4 <= 64 else (2 if vec * ch * 2 <= 64 else 1)


def k9_instance(d, vec):
    """(LPR, VEC, CH, U) of sgl_kmeans_assign_f32; CH = 0: the streaming kernel, one row per wavefront"""
    lpr = pick_lpr(d, vec)
    chunks = -(-d // (lpr * vec))
    if chunks == 1:
        ch = 1
    elif vec == 4 and chunks <= 8:
        ch = chunks if chunks <= 4 else (6 if chunks <= 6 else 8)
    elif vec == 1 and chunks <= 32:
        ch = next(c for c in (2, 4, 8, 16, 32) if chunks <= c)
    else:
        return (64, vec, 0, 1)
    return (lpr, vec, ch, k9_rows_per_group(vec, ch))


def per_batch(inst):
    """rows of one batch: (256 / LPR) x U lane groups x rows, 4 rows (one per wavefront) in a streaming kernel"""
    lpr, _, ch, u = inst
    return 4 if ch == 0 else (256 // lpr) * u


def k9_tiles(d, k, vec):
    """(tile_k, number of tiles) of launch_assign"""
    dp = -(-d // vec) * vec
    tile_k = k if k < TILE_FLOATS // dp else TILE_FLOATS // dp
    return tile_k, -(-k // tile_k)


def k9_grid(d, k, vec, n, forced=0):
    return grid(n, per_batch(k9_instance(d, vec)), CAP_K9, forced)


# ---- K12 cluster_loss_kernel ------------------------------------------------------------------------------------------------------------
def k12_instance(d, vec):
    """(LPR, VEC, CH, U) of sgl_cluster_loss_grad_f32 (cluster_loss_common.expected_instance without the tensors)"""
    lpr = pick_lpr(d, vec)
    chunks = -(-d // (lpr * vec))
    ch = 1 if chunks == 1 else next((c for c in ((2, 4, 8) if vec == 4 else (2, 8, 32)) if chunks <= c), 0)
    return (64, vec, 0, 1) if ch == 0 else (lpr, vec, ch, clc.rows_per_group(vec, ch))


def k12_tiles(d, k, vec):
    """(tile_k, number of tiles, centres of the last tile) of launch_loss"""
    dp = -(-d // vec) * vec
    tile_k = k if k <= TILE_FLOATS // dp else TILE_FLOATS // dp // K12_STEP * K12_STEP
    return tile_k, -(-k // tile_k), k - (-(-k // tile_k) - 1) * tile_k


def k12_grid(d, k, vec, n, forced=0):
    return grid(n, per_batch(k12_instance(d, vec)), CAP_K12, forced)


# ---- K14 class_loss_kernel ----------------------------------------------------------------------------------------------------------------
def k14_instance(c, vec):
    lpr, vec, ch = zlc.instance_for(c, vec)
    return (lpr, vec, ch, 1 if ch == 0 else zlc.rows_per_group(vec, ch))


def k14_grid(c, vec, n, forced=0):
    return grid(n, per_batch(k14_instance(c, vec)), CAP_K14, forced)


# ---- K11 edge_fold_kernel: one cut row per wavefront ----------------------------------------------------------------------------------------
def fold_grid(n_fold, forced=0):
    return grid(n_fold, 4, CAP_FOLD, forced)


# ---- K13 / K15: 256 / G rows per workgroup ----------------------------------------------------------------------------------------------
def pick_lanes(lanes, n_rows, nnz, nnz_b=0):
    if lanes:
        return lanes
    mean = max(nnz, nnz_b) // n_rows if n_rows > 0 else 0
    return 4 if mean < 8 else (16 if mean < 32 else 64)


def csr_grid(n_rows, lanes):
    return grid(n_rows, 256 // lanes, CAP_CSR)


# ---- stream_grid (sgl_rows.h): one thread per element, 256 per workgroup ----------------------------------------------------------------
def stream_grid(threads, agg_blocks=0):
    return grid(threads, 256, CAP_STREAM, agg_blocks)


def stream_threads(entry, n, d, n_hops=1, vec4=True, pad_cols=0, bv=8):
    """the thread count an entry point hands to stream_grid.  entry: "rows" (reduce, wsum2d, its dX, select_bwd, lincomb: n x d / vec,
    16-byte vectors iff d % 4 == 0 and every buffer is 16-byte aligned on a pitch of whole vectors), "concat4" / "concat1"
    (hop_concat_kernel<4> / <1>), "concat_any" (hop_concat_any_kernel: the output row in 16-byte vectors; pad_cols as out_cols leaves
    them), "bf16_reduce" (bv elements per thread), "bf16_concat" (4 elements per thread when vec4)"""
    if entry == "rows":
        return n * (d // 4 if vec4 else d)
    if entry == "concat4":
        return n * ((d // 4) * n_hops + pad_cols // 4)
    if entry == "concat1":
        return n * (d * n_hops + pad_cols)
    if entry == "concat_any":
        return n * ((d * n_hops + pad_cols + 3) // 4)
    if entry == "bf16_reduce":
        return n * (-(-(d + pad_cols) // bv))
    if entry == "bf16_concat":
        dw = d * n_hops + pad_cols
        return n * ((dw + 3) // 4 if vec4 else dw)
    raise ValueError(entry)


# ---- sgl_hop_wsum1d_bwd_f32 -------------------------------------------------------------------------------------------------------------
def w1d_vec(n, d):
    """(blocks, per_block) of hop_dot_partial_vec_kernel: contiguous ranges of per_block (row, vector) positions, a multiple of 256;
    per_block > 256 means every thread takes more than one"""
    total = n * ((d + 3) // 4)
    blocks = min(CAP_W1D, -(-total // 256))
    per = -(-(-(-total // blocks)) // 256) * 256
    return -(-total // per), per


def w1d_scalar_grid(n, d):
    """hop_dot_partial_kernel: a grid-stride loop over n x d elements"""
    return grid(n * d, 256, CAP_W1D)


def fill_grid(n_edges):
    """edge_fill_kernel"""
    if n_edges < FILL_FROM:
        return grid(n_edges, 256, -(-n_edges // 256) or 1)
    return grid(n_edges, 256, FILL_BLOCKS)


# ---- case lists ---------------------------------------------------------------------------------------------------------------------------
VEC_OF = {"padded": 4, "last_row": 4, "odd_view": 1}


def vec_of(layout, d, k=None):
    """floats per lane access of a kmeans_common layout; "contiguous": a plain [n, d] tensor, 16-byte lanes iff d % 4 == 0.  A single
    centre (k = 1) is passed with pitch d, so it allows 16-byte lanes only where d is a multiple of 4"""
    if k == 1 and d % 4:
        return 1
    return (4 if d % 4 == 0 else 1) if layout == "contiguous" else VEC_OF[layout]


# natural caps: n = cap x rows per batch + one more batch + a remainder (test_strided_cpu.py derives every figure)
K9_NATURAL = ((7, 7, 262273, "contiguous"), (100, 7, 65573, "padded"), (256, 7, 32787, "padded"), (1030, 17, 16395, "padded"),
              (2500, 3, 8197, "padded"))
K12_NATURAL = ((100, 7, 65573), (1030, 17, 8197), (2500, 3, 8197))             # the padded layout
FOLD_RING, FOLD_ISOLATED, FOLD_WIDTHS = 8300, 40, (7, 100)
# (lanes, rows); 131100 is a whole number of 4-row groups, so G = 64 also runs at 131102 rows, where the last group is partial
CSR_NATURAL = ((64, 131100), (64, 131102), (16, 524300), (4, 2097200))
CSR_LONG_ROW = 300
W1D_NATURAL = ((21000, 400, 3, True), (20800, 101, 3, False))                  # (n, d, H, 16-byte rows)
FILL_EDGES = 262151

# forced agg_blocks: (name, entry of stream_threads, n, d, H, 16-byte vectors, pad_cols); every thread count exceeds 4 x 256 x 3
AGG_CASES = (
    ("reduce16", "rows", 77, 200, 1, True, 0), ("reduce16", "rows", 77, 200, 4, True, 0), ("reduce_odd", "rows", 77, 147, 3, False, 0),
    ("reduce_odd", "rows", 1031, 7, 2, False, 0),
    ("wsum2d", "rows", 77, 200, 4, True, 0), ("wsum2d", "rows", 77, 147, 4, False, 0),
    ("wsum2d_dx", "rows", 77, 200, 4, True, 0), ("wsum2d_dx", "rows", 77, 147, 4, False, 0),
    ("select_bwd", "rows", 77, 200, 4, True, 0), ("select_bwd", "rows", 77, 147, 4, False, 0),
    ("lincomb", "rows", 77, 200, 4, True, 0), ("lincomb", "rows", 77, 147, 4, False, 0),
    ("concat4", "concat4", 77, 104, 4, True, 0), ("concat4", "concat4", 77, 104, 4, True, 4),
    ("concat_any", "concat_any", 1031, 7, 4, True, 0), ("concat_any", "concat_any", 1031, 7, 4, True, 4),
    ("concat1", "concat1", 1031, 3, 4, False, 0), ("concat1", "concat1", 1031, 3, 4, False, 4),
    ("bf16_reduce", "bf16_reduce", 1031, 104, 4, True, 0), ("bf16_reduce", "bf16_reduce", 77, 147, 3, False, 0),
    ("bf16_concat", "bf16_concat", 77, 104, 4, True, 0), ("bf16_concat", "bf16_concat", 1031, 7, 4, False, 0),
)


def agg_threads(case):
    name, entry, n, d, H, vec4, pad = case
    if entry == "bf16_reduce":
        return stream_threads(entry, n, d, H, vec4, pad, bv=8 if vec4 else 1)
    return stream_threads(entry, n, d, H, vec4, pad)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def k9_reference(d, k, n):
    """(x, centres, labels int64, mindist float64, near_tie bool) of kmeans_common's matrices at n rows, in float64"""
    x, c = kc.host_x(d, n), kc.host_centres(d, k, n)
    dist = kc.distances64(x, c)
    labels = dist.argmin(1)
    d1 = dist[np.arange(n), labels]
    d2 = np.partition(dist, 1, axis=1)[:, 1] if k > 1 else None
    near = (d2 - d1) <= kc.tau(d) * d2 if k > 1 else np.zeros(n, dtype=bool)
    return x, c, labels.astype(np.int64), d1, near


def row_sample(n, rows_per_batch, cap, seed=0):
    """sorted row ids: batch 0, batch cap - 1, batch cap (the first of round two), the last full batch, the partial last batch and
    2000 seeded rows"""
    full = n // rows_per_batch
    batches = [0, cap - 1, cap, full - 1] + ([full] if n % rows_per_batch else [])
    rows = [np.arange(b * rows_per_batch, min((b + 1) * rows_per_batch, n)) for b in batches if 0 <= b * rows_per_batch < n]
    rows.append(np.random.default_rng(4100 + seed).choice(n, min(SAMPLE_ROWS, n), replace=False))
    return np.unique(np.concatenate(rows))


def fold_graph():
    """(edges [E, 2], n): a ring of FOLD_RING nodes, a hub (node FOLD_RING) tied to every 7th of them, then FOLD_ISOLATED nodes
    without edges; with max_piece = 1 every ring node and the hub are cut rows"""
    ring = np.arange(FOLD_RING, dtype=np.int64)
    hub = ring[::7]
    edges = np.concatenate((np.stack((ring, (ring + 1) % FOLD_RING), 1), np.stack((np.full(len(hub), FOLD_RING), hub), 1)))
    return edges, FOLD_RING + 1 + FOLD_ISOLATED


def big_csr(n_rows, seed, long_row=None, shared_with=None, finite=False):
    """A canonical float32 CSR [n_rows, n_rows] built without a per-row loop: row i holds (i + seed) % 10 entries at columns
    base_i + j * step_i (sorted and distinct), the first and the last row are empty, row `long_row` holds CSR_LONG_ROW entries; every
    third row with entries starts at its own diagonal.  shared_with: another big_csr whose bases and steps the even rows copy, so that
    the two share columns there.  Values: random bit patterns, NaNs with payloads among them; finite: standard normal values (what a sum is
    taken of)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n_rows, dtype=np.int64)
    length = (i + seed) % 10
    length[0] = length[-1] = 0
    if long_row is not None:
        length[long_row] = CSR_LONG_ROW
    step = rng.integers(1, 8, n_rows)
    room = n_rows - (np.maximum(length, 1) - 1) * step                         # bases 0 .. room - 1 keep the row inside the matrix
    assert room.min() > 0
    base = rng.integers(0, 1 << 62, n_rows) % room
    diag = (i % 3 == 0) & (i < room)
    base[diag] = i[diag]
    if shared_with is not None:
        even = (i % 2 == 0) & (shared_with.base + (np.maximum(length, 1) - 1) * shared_with.step < n_rows)
        base[even], step[even] = shared_with.base[even], shared_with.step[even]
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(length, out=indptr[1:])
    rows = np.repeat(i, length)
    j = np.arange(indptr[-1], dtype=np.int64) - indptr[rows]
    cols = (base[rows] + j * step[rows]).astype(np.int32)
    if finite:
        data = rng.standard_normal(len(cols)).astype(np.float32)
    else:
        data = rng.integers(0, 1 << 32, len(cols), dtype=np.uint64).astype(np.uint32).view(np.float32)
    a = sp.csr_matrix((data, cols, indptr), shape=(n_rows, n_rows))
    a.base, a.step = base, step
    return a


def csr_long_row(n_rows, lanes):
    """a row of the last round of a K13 / K15 launch: the first row of the last workgroup-sized group"""
    per = 256 // lanes
    return (n_rows - 1) // per * per

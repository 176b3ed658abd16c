"""Shared by test_stream_cpu.py and test_gpu_stream_order.py (importable without a GPU): the stream-order technique and its case table.

include/sgl_hip.h promises "calls are stream-ordered and do not synchronise the device unless documented".  A test that runs a call
under a side stream, synchronises that stream and reads the result through the default stream cannot see a violation: whatever the
library put on the null stream is ordered before the very copy that checks it.  The technique here can:

  a delayed producer   S, a fresh non-blocking stream, first busy-waits for D milliseconds (delay());
  decoy inputs         the delayed inputs of a case hold a DECOY until a copy on S, behind the delay, replaces it with the real
                       values; after the call another copy on S puts the decoy back.  Anything the call put on another stream reads
                       the decoy or is overwritten (the outputs are filled with a sentinel on S behind the delay, too); a size read
                       through the host from the wrong stream is the decoy's size.  A decoy is a LEGAL input (test_stream_cpu.py
                       checks each one on numpy): a violation gives a wrong result, never a fault;
  no device-wide sync  the outputs travel to pinned host memory on S, only S is synchronised, and the host copy is compared bit for
                       bit with a plain run on the default stream.

S must have a hardware queue of its own.  A process has fewer hardware queues than streams (GPU_MAX_HW_QUEUES, 4 by default), so some
torch.cuda.Stream()s share one with the default stream: work on the two then runs in the order it was queued on both, and a launch
that went to the null stream by mistake would wait behind the delay like a correct one (measured: about one fresh stream in five).
independent_stream() therefore probes fresh streams until the default stream runs ahead of a delay on one, and keeps that one.

The mirror image runs as well (run_ahead_of_bystander): ready inputs, the call on S, and the DEFAULT stream busy for D.  What the call
queued on the null stream then happens late -- a memset wipes what a kernel on S already wrote, a kernel writes after the outputs
have travelled -- and a call that synchronises the DEVICE, not just its stream, waits for the default stream and is seen to.

Classes.  "async": right after the call returns the event recorded behind the real inputs is still pending and the call took less
host time than D / 2 -- the call neither synchronised nor outlived the delay.  "syncs": the header or the wrapper's docstring says
the call waits for the stream (a size or a plan comes back through the host): only the values decide, and the event must still
be pending just BEFORE the call.  The quote that documents it is part of the table (test_stream_cpu.py looks it up).

Decoys: float32 / bfloat16 / float64 arrays are filled with 0x7FC07FC0 (a NaN as float32 and as two bfloat16, a finite 2^1021-ish
float64); index lists (gather indices, labels, edge lists, permutations, COO rows and columns) are rotations of the real list; CSR
columns keep their row pointers and become n_cols - 1 - col, reversed inside each row (strictly increasing, in range); a decoy row
pointer array (sgl_csr_create only, which builds its plan from it) is monotone with the same n and the same nnz.

The table holds one case per function of include/sgl_hip.h and include/sgl_probe.h whose last parameter is `void *stream`, minus
EXCLUDED (reasons there); test_stream_cpu.py proves that by parsing the headers.  Shapes: N = 1031 rows (more than one workgroup,
no multiple of any tile), d in WIDTHS = (24, 100), H = 4 hops, a graph with a hub row above the default long_row_nnz bracket (the
SpMM fix-up kernel launches), an ingest list with duplicate pairs, an edge list with a folded hub row."""
import atexit
import ctypes
import functools
import re
import time
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

N, H = 1031, 4
WIDTHS = (24, 100)
HUB = 7
K_CENTRES = 7
FILL32 = 0x7FC07FC0
DELAY_FLOOR_MS = 20.0                # D = max(4 x the largest t_plain of an async case, this)
T_PLAIN_FACTOR = 4.0

# header functions that end in `void *stream)` and have no case, with the reason
EXCLUDED = {
    "sgl_allgather_rows": "moves rows between ranks: needs a communicator of more than one rank (world == 1 is a no-op)",
    "sgl_exchange_rows": "moves rows between ranks: needs a communicator of more than one rank",
    "sgl_probe_stream_f32": "a measurement probe that writes nothing: there is no output a mis-queued launch could change",
    "sgl_probe_gather_f32": "a measurement probe that writes nothing: there is no output a mis-queued launch could change",
}
# sgl_spmm_multi_f32 is in the table in its single-GPU form (two local replicas); peer pointers need a second GPU.

Delayed = namedtuple("Delayed", "real decoy kind info")


# ---- decoys ---------------------------------------------------------------------------------------------------------------------------
def nan_like(a):
    """an array of a's shape and dtype whose bytes are FILL32 repeated"""
    a = np.ascontiguousarray(a)
    assert a.nbytes % 4 == 0, "a decoy is filled in 32-bit words"
    return np.full(a.nbytes // 4, FILL32, dtype=np.uint32).view(a.dtype).reshape(a.shape)


def rotated(a, k=1):
    """the list rotated by k places along its first axis: the same values, hence in range wherever the list was"""
    return np.ascontiguousarray(np.roll(a, k, axis=0))


def decoy_col(rowptr, col, n_cols):
    """n_cols - 1 - col, reversed inside each row: strictly increasing where col was, in [0, n_cols)"""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    q = rowptr[rows] + rowptr[rows + 1] - 1 - np.arange(len(col))
    return (n_cols - 1 - col[q]).astype(col.dtype)


def decoy_rowptr(rowptr):
    """the nnz entries spread evenly over the rows: monotone, n + 1 offsets, the same nnz -- and no long row"""
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    return (np.arange(n + 1, dtype=np.int64) * nnz // n).astype(np.int64)


def fl(real):
    return Delayed(np.ascontiguousarray(real), nan_like(real), "float", {})


def ix(real, hi, k=1):
    return Delayed(np.ascontiguousarray(real), rotated(real, k), "index", {"hi": int(hi)})


def cc(rowptr, col, n_cols):
    return Delayed(col, decoy_col(rowptr, col, n_cols), "csr_col", {"rowptr": rowptr, "n_cols": int(n_cols)})


def rp(rowptr):
    return Delayed(rowptr, decoy_rowptr(rowptr), "rowptr", {})


def legal(dl):
    """None if the decoy of a Delayed is a legal input that differs from the real one, else what is wrong with it"""
    real, decoy = dl.real, dl.decoy
    if real.shape != decoy.shape or real.dtype != decoy.dtype:
        return "shape or dtype differs"
    if real.tobytes() == decoy.tobytes():
        return "the decoy equals the real input"
    if dl.kind == "index":
        if decoy.min() < 0 or decoy.max() >= dl.info["hi"]:
            return "index out of range"
    elif dl.kind == "csr_col":
        rowptr, n_cols = dl.info["rowptr"], dl.info["n_cols"]
        if len(decoy) and (decoy.min() < 0 or decoy.max() >= n_cols):
            return "column out of range"
        inner = np.ones(len(decoy), dtype=bool)
        inner[rowptr[:-1][np.diff(rowptr) > 0]] = False                       # the first entry of a row has no predecessor
        if not np.all(np.diff(decoy.astype(np.int64), prepend=-1)[inner] > 0):
            return "a row is not strictly increasing"
    elif dl.kind == "rowptr":
        if decoy[0] != 0 or decoy[-1] != real[-1] or np.any(np.diff(decoy) < 0):
            return "not a monotone row pointer array with the same nnz"
    elif dl.kind != "float":
        return f"unknown kind {dl.kind}"
    return None


# ---- host inputs ----------------------------------------------------------------------------------------------------------------------
Graph = namedtuple("Graph", "rowptr col val n nnz")


@functools.lru_cache(maxsize=None)
def graph(seed=7, diagonal=3):
    """A symmetric canonical float32 CSR [N, N] with positive weights: a ring, three random neighbours per node, a hub (row HUB tied
    to every third node: above the long_row_nnz bracket of a matrix this small, 32) and a stored diagonal on every `diagonal`-th row
    (1: every row, the pattern of A + I)."""
    rng = np.random.default_rng(seed)
    i = np.arange(N, dtype=np.int64)
    r = np.concatenate((i, np.repeat(i, 3), np.full(len(i[::3]), HUB)))
    c = np.concatenate(((i + 1) % N, rng.integers(0, N, 3 * N), i[::3]))
    keep = r != c
    r, c = r[keep], c[keep]
    dg = i[::diagonal]
    r, c = np.concatenate((r, c, dg)), np.concatenate((c, r, dg))
    a = sp.coo_matrix((np.ones(len(r), dtype=np.float32), (r, c)), shape=(N, N)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    rows = np.repeat(i, np.diff(a.indptr))
    lo, hi = np.minimum(rows, a.indices), np.maximum(rows, a.indices)
    val = (0.25 + ((lo * 31 + hi * 17) % 13) / 16.0).astype(np.float32)          # symmetric, exact in float32
    g = Graph(a.indptr.astype(np.int64), a.indices.astype(np.int32), val, N, int(a.nnz))
    assert g.nnz < (1 << 18) and np.diff(g.rowptr).max() > 4 * 32 and np.diff(g.rowptr).min() >= 2
    return g


def missing_diagonal(g):
    rows = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    return g.n - int(np.count_nonzero(rows == g.col))


def diag_positions(g):
    rows = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    pos = np.full(g.n, -1, dtype=np.int64)
    at = np.flatnonzero(rows == g.col)
    pos[rows[at]] = at
    return pos


@functools.lru_cache(maxsize=None)
def feats(d, salt=0):
    """H float32 [N, d] hop matrices"""
    rng = np.random.default_rng(1000 * d + salt)
    return tuple(rng.standard_normal((N, d)).astype(np.float32) for _ in range(H))


def bf16_bits(a):
    """float32 -> the uint16 patterns of its truncation to bfloat16"""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def vec(d, salt, parts=1, tail=False):
    """`parts` weight vectors of d floats, each zero-padded to whole 16-byte vectors (+ 4 floats holding a bias when tail)"""
    dp = (d + 3) // 4 * 4
    rng = np.random.default_rng(77 * d + salt)
    v = np.zeros(parts * dp + (4 if tail else 0), dtype=np.float32)
    for p in range(parts):
        v[p * dp:p * dp + d] = rng.standard_normal(d).astype(np.float32) / np.float32(d)
    return v


@functools.lru_cache(maxsize=None)
def gather_index():
    rng = np.random.default_rng(3)
    return rng.integers(0, N, 777).astype(np.int64)


@functools.lru_cache(maxsize=None)
def edge_list():
    """int64 [E, 2]: 600 random pairs and 120 pairs at HUB, alternating sides (with max_piece = 32 its row is folded)"""
    rng = np.random.default_rng(9)
    e = rng.integers(0, N, (600, 2)).astype(np.int64)
    hub = np.stack((np.full(120, HUB, dtype=np.int64), (np.arange(120, dtype=np.int64) * 5) % N), 1)
    hub[1::2] = hub[1::2, ::-1]
    return np.ascontiguousarray(np.concatenate((e, hub)))


@functools.lru_cache(maxsize=None)
def coo_list():
    """(row, col, val): the entries of graph() in a shuffled order, every seventh stored a second time (duplicate pairs)"""
    g = graph()
    rows = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.rowptr))
    r, c, v = np.concatenate((rows, rows[::7])), np.concatenate((g.col, g.col[::7])).astype(np.int64), np.concatenate((g.val, g.val[::7]))
    p = np.random.default_rng(13).permutation(len(r))
    return r[p], c[p], v[p]


# ---- the case table --------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "entry klass via widths host setup doc inputless oracle waits")
CASES = {}


def case(entry, klass="async", via="device._call", widths=WIDTHS, doc=None, inputless=False, oracle=None, waits=None):
    """register `setup` (below the decorator) with `host` = setup.host; doc: (where, quote) for a syncs case -- where is "header" or
    the dotted name of the wrapper whose docstring holds the quote; waits: what a syncs case is documented to wait for, "stream"
    (its own stream alone: with only the default stream busy the call returns at once) or "device" (it frees temporaries with
    hipFree, which waits for every stream: the call is seen to wait for the busy default stream).  An async case waits for nothing.
    A case that goes through device._call and not through a wrapper says why in CALL_REASONS."""
    def deco(cls):
        assert entry not in CASES and klass in ("async", "syncs") and (klass == "async" or doc)
        assert waits == (None if klass == "async" else waits) and (klass == "async" or waits in ("stream", "device"))
        CASES[entry] = Case(entry, klass, via, widths, cls.host, cls.setup, doc, inputless, oracle or getattr(cls, "oracle", None), waits)
        return cls
    return deco


# why a case calls the entry point through device._call (the product's call path: it appends the current stream) and not through a
# device.py wrapper
_PAIR = ("the wrapper (device.{0}) makes both calls of the pair in one: the table takes them apart so that each is classified on its "
         "own, and the wrapper runs in the transforms flows")
_NORM = ("the wrappers (PreparedAdjacency, PreparedBlock, normalize_adj) chain several entry points with host reads and caches "
         "between them: one case per entry point needs the call alone; the propagate flows run the wrappers")
_AUTOGRAD = "reached only from inside a torch.autograd.Function ({0}): the case needs the launch alone, on outputs it can poison"
CALL_REASONS = {
    "sgl_hop_concat_f32": "the wrapper (hop_concat) launches the padded form; nothing in device.py calls the un-suffixed entry point",
    "sgl_nafs_f32": "the wrapper (nafs_aggregate) launches the padded form; nothing in device.py calls the un-suffixed entry point",
    "sgl_gather_rows_f32": "the wrapper (gather_rows) launches the padded form; nothing in device.py calls the un-suffixed entry point",
    "sgl_hop_gate_f32": "the wrapper (hop_gate) launches the padded form; nothing in device.py calls the un-suffixed entry point",
    "sgl_hop_wsum1d_bwd_f32": _AUTOGRAD.format("_WSum1D.backward"),
    "sgl_hop_select_bwd_f32": _AUTOGRAD.format("_ReduceGrad.backward"),
    "sgl_hop_gate_padded_f32": _AUTOGRAD.format("_GateFused, which also takes the gate's parameters as tensors that require grad"),
    "sgl_hop_recursive_f32": _AUTOGRAD.format("_RecursiveFused"),
    "sgl_hop_recursive_bwd_f32": _AUTOGRAD.format("_RecursiveFused.backward"),
    "sgl_hop_rowdot2_f32": _AUTOGRAD.format("_HopScores2"),
    "sgl_download": "the wrapper (download_rows) copies through torch below 8 MiB and reaches the entry point only above",
    "sgl_exchange_selftest": "no wrapper: a check for C callers",
    "sgl_edge_loss_grad_f32": "the wrapper (edge_loss_grad) takes an EdgePlan, which keeps its output buffers to itself; the tables here "
                              "are edge_loss_common's, the outputs are poisoned, and the wrapper runs in the edge_bce_loss flows",
    "sgl_csr_select_rowptr": _PAIR.format("csr_select"), "sgl_csr_select_fill": _PAIR.format("csr_select"),
    "sgl_csr_merge_rowptr": _PAIR.format("csr_merge"), "sgl_csr_merge_fill": _PAIR.format("csr_merge"),
    "sgl_coo_to_csr": "the wrapper (io.coo_to_csr_device) clones the valid prefix of its outputs into tensors of its own: the case poisons "
                      "the arrays the entry point writes; the wrapper runs in the to_undirected and mask_test_edges flows",
    "sgl_reorder_lpa_round": "called by dist/redistribute.py between all-gathers of a process group only",
    "sgl_norm_degrees": "no wrapper: the degrees of a row block for C callers (the Python layer takes them from sgl_norm_block_build)",
    "sgl_norm_block_colsum": "reached only for a directed block inside PreparedBlock.__init__, between host reads",
    "sgl_norm_block_mix": "no wrapper calls it: _scaled_values uses the flat form, sgl_norm_block_mix_at",
}
CALL_REASONS.update({e: _NORM for e in ("sgl_norm_prepare", "sgl_norm_block_prepare", "sgl_norm_execute", "sgl_norm_execute_lr",
                                        "sgl_norm_block_build", "sgl_norm_build_symcheck", "sgl_norm_block_scale", "sgl_norm_block_mix_at",
                                        "sgl_norm_block_diag_positions", "sgl_norm_degree_powers")})


def case_ids():
    return [(e, d) for e, c in CASES.items() for d in c.widths]


def spmm_oracle(h):
    g = graph()
    a = sp.csr_matrix((g.val.astype(np.float64), h["col"], g.rowptr), shape=(N, N))
    return a @ h["x"].astype(np.float64)


class _Spmm:
    """the SpMM family: X delayed (NaN decoy), the handle built in setup from ready arrays"""
    bf16 = False

    @classmethod
    def host(cls, d):
        g = graph()
        x = feats(d)[0]
        return {"rowptr": g.rowptr, "col": g.col, "val": g.val, "x": fl(bf16_bits(x) if cls.bf16 else x),
                "res": feats(d, 1)[1], "acc0": feats(d, 2)[2]}

    @staticmethod
    def handle(t):
        t.csr = t.dev.DeviceCSR(t.rowptr, t.col, t.val, (N, N))
        assert t.csr.info()["n_long_rows"] >= 1, "the fix-up kernel must launch"
        return t.csr


@case("sgl_spmm_f32", via="DeviceCSR.spmm")
class _(_Spmm):
    @staticmethod
    def setup(t):
        csr, o = _Spmm.handle(t), t.out_rows(N, t.x.shape[1])
        return lambda: [csr.spmm(t.x, out=o)]

    @staticmethod
    def oracle(h):
        return spmm_oracle({"col": graph().col, "x": h["x"]})


@case("sgl_spmm_multi_f32", via="DeviceCSR.spmm_multi")
class _(_Spmm):
    @staticmethod
    def setup(t):
        csr, d = _Spmm.handle(t), t.x.shape[1]
        o = [t.out_rows(N, d), t.out_rows(N, d)]

        def call():
            csr.spmm_multi(t.x, [q.data_ptr() for q in o], o[0].stride(0))
            return o
        return call


@case("sgl_spmm_chain_f32", via="DeviceCSR.spmm_chain")
class _(_Spmm):
    @staticmethod
    def setup(t):
        csr, o = _Spmm.handle(t), [t.out_rows(N, t.x.shape[1]) for _ in range(3)]
        return lambda: csr.spmm_chain(t.x, 3, outs=o)


@case("sgl_chain_graph_launch", via="ChainGraph.replay")
class _(_Spmm):
    @staticmethod
    def setup(t):
        csr, o = _Spmm.handle(t), [t.out_rows(N, t.x.shape[1]) for _ in range(3)]
        t.graph = csr.capture_chain(t.x, o)             # sgl_chain_graph_create: runs the chain once and synchronises, here in setup
        return lambda: t.graph.replay()


@case("sgl_spmm_axpb_clamp_f32", via="DeviceCSR.spmm_axpb_clamp")
class _(_Spmm):
    @staticmethod
    def setup(t):
        csr, o = _Spmm.handle(t), t.out_rows(N, t.x.shape[1])
        return lambda: [csr.spmm_axpb_clamp(t.x, 0.9, res=t.res, lo=-1.0, hi=1.0, out=o)]


@case("sgl_spmm_acc_f32", via="DeviceCSR.spmm_acc")
class _(_Spmm):
    @staticmethod
    def setup(t):
        csr, o, acc = _Spmm.handle(t), t.out_rows(N, t.x.shape[1]), t.inout(t.acc0)
        return lambda: [csr.spmm_acc(t.x, o, acc, mode="sum"), acc]


class _SpmmBf16(_Spmm):
    bf16 = True


@case("sgl_spmm_bf16", via="DeviceCSR.spmm")
class _(_SpmmBf16):
    @staticmethod
    def setup(t):
        csr, o = _Spmm.handle(t), t.out_rows(N, t.x.shape[1], bf16=True)
        return lambda: [csr.spmm(t.x, out=o)]


@case("sgl_spmm_chain_bf16", via="DeviceCSR.spmm_chain")
class _(_SpmmBf16):
    @staticmethod
    def setup(t):
        csr, o = _Spmm.handle(t), [t.out_rows(N, t.x.shape[1], bf16=True) for _ in range(3)]
        return lambda: csr.spmm_chain(t.x, 3, outs=o)


@case("sgl_spmm_acc_bf16", via="DeviceCSR.spmm_acc")
class _(_SpmmBf16):
    @staticmethod
    def setup(t):
        csr, o, acc = _Spmm.handle(t), t.out_rows(N, t.x.shape[1], bf16=True), t.inout(t.acc0)
        return lambda: [csr.spmm_acc(t.x, o, acc, w=0.5, mode="wsum"), acc]


@case("sgl_csr_create", "syncs", via="DeviceCSR", widths=(None,),
      doc=("header", "copies the row pointers to the host once: this call synchronises `stream`"), waits="stream")
class _:
    """the plan is built from whichever row pointers the call saw: its counts come back through sgl_csr_info"""
    @staticmethod
    def host(d):
        g = graph()
        return {"rowptr": rp(g.rowptr), "col": g.col, "val": g.val}

    @staticmethod
    def setup(t):
        def call():
            t.csr = t.dev.DeviceCSR(t.rowptr, t.col, t.val, (N, N))
            i = t.csr.info()
            return [t.torch.tensor([i["n_items"], i["n_pieces"], i["n_long_rows"]], dtype=t.torch.int64)]
        return call


@case("sgl_csr_set_rowmap", "syncs", via="DeviceCSR.set_rowmap", widths=(24,),
      doc=("header", "the scratch of the validation is freed on return: this call synchronises the DEVICE"), waits="device")
class _:
    """the split rows' output ids are read from the map when it is set: the product through the map shows which map that was"""
    @staticmethod
    def host(d):
        g = graph()
        perm = np.random.default_rng(21).permutation(N).astype(np.int32)
        return {"rowptr": g.rowptr, "col": g.col, "val": g.val, "x": feats(d)[0], "rowmap": ix(perm, N, 5)}

    @staticmethod
    def setup(t):
        csr, o = _Spmm.handle(t), t.out_rows(N, t.x.shape[1])

        def call():
            csr.set_rowmap(t.rowmap)
            return [csr.spmm(t.x, out=o)]
        return call


class _Hops:
    """the aggregators: every hop matrix delayed (NaN decoy)"""
    bf16 = False

    @classmethod
    def host(cls, d):
        h = {f"x{k}": fl(bf16_bits(f) if cls.bf16 else f) for k, f in enumerate(feats(d))}
        rng = np.random.default_rng(5 * d)
        h.update(w2=rng.random((N, H)).astype(np.float32), w1=rng.random(H).astype(np.float32) + np.float32(0.5),
                 gout=feats(d, 3)[0], gw=rng.standard_normal((N, H)).astype(np.float32), idx=gather_index(),
                 lin=np.array([[1, 0, .5, 0], [0, 2, 0, -1], [.25, .25, .25, .25]], dtype=np.float32),
                 v1=vec(d, 1), v1t=vec(d, 1, tail=True), v2t=vec(d, 2, parts=2, tail=True), u=feats(d, 4)[0][:H].copy())
        return h

    @staticmethod
    def hops(t):
        return [getattr(t, f"x{k}") for k in range(H)]


class _HopsBf16(_Hops):
    bf16 = True


def hops_case(entry, via="device._call", bf16=False, **kw):
    """a case over the hop list: the decorated function is setup(t, hops)"""
    def deco(fn):
        base = _HopsBf16 if bf16 else _Hops
        cls = type("_", (base,), {"setup": staticmethod(lambda t: fn(t, base.hops(t)))})
        return case(entry, via=via, **kw)(cls)
    return deco


@hops_case("sgl_hop_reduce_f32", via="device.hop_reduce", oracle=lambda h: sum(h[f"x{k}"].astype(np.float64) for k in range(H)))
def _(t, x):
    return lambda: [t.dev.hop_reduce(t.lib.SGL_REDUCE_SUM, x)]


@hops_case("sgl_hop_reduce_bf16_f32", via="device.hop_reduce", bf16=True)
def _(t, x):
    return lambda: [t.dev.hop_reduce(t.lib.SGL_REDUCE_WSUM, x, t.w1)]


@hops_case("sgl_hop_concat_padded_f32", via="device.hop_concat", oracle=lambda h: np.hstack([h[f"x{k}"] for k in range(H)]))
def _(t, x):
    return lambda: [t.dev.hop_concat(x)]


@hops_case("sgl_hop_concat_f32")
def _(t, x):
    n, d = x[0].shape
    o = t.out_rows(n, H * d)
    ptrs, lds = t.lib.hop_arrays(x)

    def call():
        t.call("sgl_hop_concat_f32", H, ptrs, lds, t.ptr(o), o.stride(0), n, d)
        return [o]
    return call


@hops_case("sgl_hop_concat_bf16", via="device.hop_concat", bf16=True)
def _(t, x):
    return lambda: [t.dev.hop_concat(x, out_dtype=t.torch.bfloat16)]


@hops_case("sgl_hop_concat_bf16_f32", via="device.hop_concat", bf16=True)
def _(t, x):
    return lambda: [t.dev.hop_concat(x)]


@hops_case("sgl_hop_lincomb_f32", via="device.hop_lincomb")
def _(t, x):
    return lambda: t.dev.hop_lincomb(x, t.lin)


@hops_case("sgl_hop_wsum2d_f32", via="device.hop_wsum2d")
def _(t, x):
    return lambda: [t.dev.hop_wsum2d(x, t.w2)]


@hops_case("sgl_hop_wsum2d_bwd_f32", via="device._wsum2d_backward")
def _(t, x):
    def call():
        dw, dxs = t.dev._wsum2d_backward(t.w2, x, t.gout, True, [True] * H)
        return [dw] + dxs
    return call


@hops_case("sgl_hop_rowdot_f32", via="device.hop_scores")
def _(t, x):
    v = t.v1[:x[0].shape[1]]
    return lambda: [t.dev.hop_scores(x, v)]


@hops_case("sgl_hop_wsum1d_bwd_f32")
def _(t, x):
    n, d = x[0].shape
    dw = t.out(H)
    scratch = t.out(int(t.call("sgl_hop_wsum1d_bwd_scratch", H, raw=True)), poison=False)
    ptrs, lds = t.lib.hop_arrays(x)

    def call():
        t.call("sgl_hop_wsum1d_bwd_f32", H, ptrs, lds, t.ptr(t.gout), t.gout.stride(0), t.ptr(dw), t.ptr(scratch), n, d)
        return [dw]
    return call


@hops_case("sgl_hop_select_bwd_f32")
def _(t, x):
    n, d = x[0].shape
    dx = [t.out_rows(n, d) for _ in range(H)]
    ptrs, lds = t.lib.hop_arrays(x)
    dptrs, dlds = t.lib.hop_arrays(dx)

    def call():
        t.call("sgl_hop_select_bwd_f32", t.lib.SGL_REDUCE_MAX, H, ptrs, lds, t.ptr(t.gout), t.gout.stride(0), dptrs, dlds, n, d)
        return dx
    return call


@hops_case("sgl_nafs_f32")
def _(t, x):
    n, d = x[0].shape
    o, w = t.out_rows(n, d), t.out(n, H)
    ptrs, lds = t.lib.hop_arrays(x)

    def call():
        t.call("sgl_nafs_f32", H, ptrs, lds, t.ptr(o), o.stride(0), t.ptr(w), H, n, d)
        return [o, w]
    return call


@hops_case("sgl_nafs_padded_f32", via="device.nafs_aggregate")
def _(t, x):
    return lambda: list(t.dev.nafs_aggregate(x, return_weights=True))


@hops_case("sgl_nafs_bf16_f32", via="device.nafs_aggregate", bf16=True)
def _(t, x):
    return lambda: list(t.dev.nafs_aggregate(x, return_weights=True))


@hops_case("sgl_nafs_prefix_f32", via="device.nafs_prefix")
def _(t, x):
    return lambda: t.dev.nafs_prefix(x, [1, 3])


def _gate_outputs(t, n, d):
    return t.out_rows(n, d), t.out(n, H), t.out(n, H)


@hops_case("sgl_hop_gate_f32")
def _(t, x):
    n, d = x[0].shape
    o, w, g = _gate_outputs(t, n, d)
    ptrs, lds = t.lib.hop_arrays(x)

    def call():
        t.call("sgl_hop_gate_f32", H, ptrs, lds, t.ptr(t.v1), 0.125, t.ptr(o), o.stride(0), t.ptr(w), H, t.ptr(g), H, n, d)
        return [o, w, g]
    return call


@hops_case("sgl_hop_gate_padded_f32")
def _(t, x):
    n, d = x[0].shape
    o, w, g = _gate_outputs(t, n, d)
    ptrs, lds = t.lib.hop_arrays(x)
    pad = t.dev.own_pad(o)

    def call():     # bias = NaN: read from the device, behind the padded vector
        t.call("sgl_hop_gate_padded_f32", H, ptrs, lds, t.ptr(t.v1t), float("nan"), t.ptr(o), o.stride(0), pad, t.ptr(w), H, t.ptr(g), H, n, d)
        return [o, w, g]
    return call


@hops_case("sgl_hop_recursive_f32")
def _(t, x):
    n, d = x[0].shape
    o, w, a, c = t.out_rows(n, d), t.out(n, H), t.out(n, H), t.out(n, H)
    ptrs, lds = t.lib.hop_arrays(x)
    pad = t.dev.own_pad(o)

    def call():
        t.call("sgl_hop_recursive_f32", H, ptrs, lds, t.ptr(t.v2t), float("nan"), t.ptr(o), o.stride(0), pad, t.ptr(w), H, t.ptr(a), H,
               t.ptr(c), H, n, d)
        return [o, w, a, c]
    return call


@hops_case("sgl_hop_colsum_f32", via="device.hop_colsum")
def _(t, x):
    return lambda: [t.dev.hop_colsum(x, t.w2)]


@hops_case("sgl_hop_rowdot2_f32")
def _(t, x):
    n, d = x[0].shape
    dp = (d + 3) // 4 * 4
    u = t.torch.zeros((H, dp), dtype=t.torch.float32, device=t.device)
    u[:, :d] = t.u
    p, a = t.out(n, H - 1), t.out(n)
    ptrs, lds = t.lib.hop_arrays(x)

    def call():
        t.call("sgl_hop_rowdot2_f32", H, ptrs, lds, t.ptr(u), dp, 0b0101, t.ptr(t.v1), 1, H, t.ptr(p), H - 1, t.ptr(a), n, d)
        return [p, a]
    return call


@hops_case("sgl_gather_hops_padded_f32", via="device.gather_hops")
def _(t, x):
    return lambda: t.dev.gather_hops(x, t.idx)


@hops_case("sgl_gather_hops_bf16_f32", via="device.gather_hops", bf16=True)
def _(t, x):
    return lambda: t.dev.gather_hops(x, t.idx)


@case("sgl_hop_recursive_bwd_f32")
class _:
    @staticmethod
    def host(d):
        rng = np.random.default_rng(31 + d)
        return {k: fl(rng.standard_normal((N, H)).astype(np.float32) / np.float32(4)) for k in ("a", "c", "gw")}

    @staticmethod
    def setup(t):
        da, dc, db = t.out(N, H), t.out(N, H), t.out(N)

        def call():
            t.call("sgl_hop_recursive_bwd_f32", H, t.ptr(t.a), H, t.ptr(t.c), H, 0.125, None, t.ptr(t.gw), H, t.ptr(da), H, t.ptr(dc), H,
                   t.ptr(db), N)
            return [da, dc, db]
        return call


class _Gather:
    """x[idx]: the matrix (NaN decoy) and the index list (rotated) are both delayed"""
    bf16 = False

    @classmethod
    def host(cls, d):
        x = feats(d)[0]
        dst = np.random.default_rng(17).permutation(len(gather_index())).astype(np.int64)
        return {"x": fl(bf16_bits(x) if cls.bf16 else x), "idx": ix(gather_index(), N, 3), "dst": dst}

    @staticmethod
    def oracle(h):
        return h["x"][h["idx"]]


@case("sgl_gather_rows_f32")
class _(_Gather):
    @staticmethod
    def setup(t):
        m, d = t.idx.numel(), t.x.shape[1]
        o = t.out_rows(m, d)

        def call():
            t.call("sgl_gather_rows_f32", t.ptr(t.x), t.x.stride(0), N, t.ptr(t.idx), m, t.ptr(o), o.stride(0), d)
            return [o]
        return call


@case("sgl_gather_rows_padded_f32", via="device.gather_rows")
class _(_Gather):
    @staticmethod
    def setup(t):
        return lambda: [t.dev.gather_rows(t.x, t.idx)]


@case("sgl_gather_rows_bf16_f32", via="device.gather_rows")
class _(_Gather):
    bf16 = True
    oracle = None

    @staticmethod
    def setup(t):
        return lambda: [t.dev.gather_rows(t.x, t.idx)]


@case("sgl_scatter_rows_f32", via="device.scatter_rows")
class _(_Gather):
    @staticmethod
    def setup(t):
        o = t.out_rows(t.idx.numel(), t.x.shape[1])
        return lambda: [t.dev.scatter_rows(t.x, t.idx, t.dst, o)]

    @staticmethod
    def oracle(h):
        o = np.zeros((len(h["idx"]), h["x"].shape[1]), dtype=np.float32)
        o[h["dst"]] = h["x"][h["idx"]]
        return o


@case("sgl_col_signature_f32", via="device.column_signature")
class _(_Gather):
    oracle = None

    @staticmethod
    def setup(t):
        return lambda: [t.dev.column_signature(t.x)]


@case("sgl_download", "syncs", widths=(100,), doc=("header", "Synchronous; waits for `stream` (the producer) first"), waits="stream")
class _:
    @staticmethod
    def host(d):
        return {"src": fl(feats(d)[0].reshape(-1))}

    @staticmethod
    def setup(t):
        host = t.torch.zeros(t.src.numel(), dtype=t.torch.float32)

        def call():
            t.call("sgl_download", host.data_ptr(), t.ptr(t.src), t.src.numel() * 4)
            return [host]
        return call


@case("sgl_exchange_selftest", widths=(100,))
class _:
    """on a one-rank communicator of the real librccl (skipped without it, as test_gpu_parity.py does)"""
    @staticmethod
    def host(d):
        return {"src": fl(feats(d)[1].reshape(-1))}

    @staticmethod
    def setup(t):
        comm = one_rank_communicator()
        o = t.out(t.src.numel())

        def call():
            t.call("sgl_exchange_selftest", comm, 0, t.ptr(t.src), t.ptr(o), t.src.numel(), 3)
            return [o]
        return call


# ---- edges, losses -------------------------------------------------------------------------------------------------------------------
@case("sgl_edge_dot_f32", via="device.edge_dot")
class _:
    @staticmethod
    def host(d):
        return {"z": fl(feats(d)[0]), "edges": ix(edge_list(), N, 11)}

    @staticmethod
    def setup(t):
        return lambda: [t.dev.edge_dot(t.z, t.z, t.edges)]

    @staticmethod
    def oracle(h):
        z = h["z"].astype(np.float64)
        return (z[h["edges"][:, 0]] * z[h["edges"][:, 1]]).sum(1)


@case("sgl_edge_loss_grad_f32")
class _:
    """the prepared tables of edge_loss_common.plan_tables with max_piece = 32: HUB's row is cut and folded"""
    @staticmethod
    def host(d):
        import edge_loss_common as elc
        e = edge_list()
        _, other, code, pieces, fold, n_partial = elc.plan_tables(e, N, 32)
        assert len(fold) >= 1 and n_partial >= 2
        y = (np.arange(len(e)) % 3 == 0).astype(np.float32)
        return {"z": fl(feats(d)[0] / np.float32(8)), "other": other, "code": code, "pieces": pieces, "fold": fold, "labels": y,
                "n_partial": np.array([n_partial], dtype=np.int64)}

    @staticmethod
    def setup(t):
        n, d = t.z.shape
        n_e, n_p, n_f, n_partial = t.labels.numel(), t.pieces.shape[0], t.fold.shape[0], int(t.host["n_partial"][0])
        dz, score, coef, loss = t.out_rows(n, d), t.out(n_e), t.out(n_e), t.out(n_p)
        partial = t.dev.alloc_rows(n_partial, d, t.device)

        def call():
            t.call("sgl_edge_loss_grad_f32", t.ptr(t.z), t.z.stride(0), n, d, t.ptr(t.pieces), n_p, t.ptr(t.other), t.ptr(t.code), 2 * n_e,
                   t.ptr(t.labels), None, n_e, 1, 1.0 / n_e, t.ptr(dz), dz.stride(0), t.ptr(partial), partial.stride(0), n_partial,
                   t.ptr(t.fold), n_f, t.ptr(score), t.ptr(coef), t.ptr(loss))
            return [dz, score, coef, loss]
        return call


@case("sgl_kmeans_assign_f32", via="device.kmeans_assign")
class _:
    @staticmethod
    def host(d):
        return {"x": fl(feats(d)[0]), "centres": feats(d, 6)[1][:K_CENTRES].copy()}

    @staticmethod
    def setup(t):
        return lambda: list(t.dev.kmeans_assign(t.x, t.centres))

    @staticmethod
    def oracle(h):
        x, c = h["x"].astype(np.float64), h["centres"].astype(np.float64)
        dist = ((x[:, None, :] - c[None, :, :]) ** 2).sum(2)
        return np.where(np.isnan(dist).all(1), 0, np.argmin(np.where(np.isnan(dist), np.inf, dist), 1))


@case("sgl_cluster_loss_grad_f32", via="device.cluster_loss_grad")
class _:
    @staticmethod
    def host(d):
        y = (np.arange(N, dtype=np.int64) * 3) % K_CENTRES
        return {"x": fl(feats(d)[0]), "centres": feats(d, 6)[1][:K_CENTRES].copy(), "labels": ix(y, K_CENTRES, 1)}

    @staticmethod
    def setup(t):
        return lambda: list(t.dev.cluster_loss_grad(t.x, t.centres, t.labels, 1.0 / N, dx=True, row_loss=True))


@case("sgl_class_loss_grad_f32", via="device.class_loss_grad")
class _:
    @staticmethod
    def host(d):
        y = (np.arange(N, dtype=np.int64) * 5) % d
        return {"z": fl(feats(d)[0]), "labels": ix(y, d, 1)}

    @staticmethod
    def setup(t):
        return lambda: list(t.dev.class_loss_grad(t.z, t.labels, 1.0 / N, dz=True, row_loss=True, pred=True))

    @staticmethod
    def oracle(h):
        z = h["z"].astype(np.float64)
        m = z.max(1, keepdims=True)
        return (m[:, 0] + np.log(np.exp(z - m).sum(1))) - z[np.arange(N), h["labels"]]


# ---- CSR structure: search, candidates, select, merge, ingest, reorder ----------------------------------------------------------------------
def _adj(t, col=None):
    return SimpleNamespace(rowptr=t.rowptr, col=t.col if col is None else col, val=getattr(t, "val", None), shape=(N, N))


@case("sgl_csr_find", via="device.csr_find", widths=(None,))
class _:
    @staticmethod
    def host(d):
        g = graph()
        rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(g.rowptr))
        q = np.stack((rows[::3], g.col[::3].astype(np.int64)), 1)                  # stored pairs ...
        q = np.concatenate((q, edge_list()))                                        # ... and mostly missing ones
        return {"rowptr": g.rowptr, "col": cc(g.rowptr, g.col, N), "edges": ix(q, N, 7)}

    @staticmethod
    def setup(t):
        return lambda: [t.dev.csr_find(_adj(t), t.edges)]

    @staticmethod
    def oracle(h):
        g = graph()
        where = {(int(r), int(c)): p for p, (r, c) in enumerate(zip(np.repeat(np.arange(N), np.diff(g.rowptr)), h["col"]))}
        return np.array([where.get((int(u), int(v)), -1) for u, v in h["edges"]], dtype=np.int64)


@case("sgl_edge_candidates", via="device.edge_candidates", widths=(None,))
class _:
    """the candidates do not depend on the matrix, their keys do: a dense block of stored pairs makes many verdicts differ"""
    @staticmethod
    def host(d):
        g = graph()
        return {"rowptr": g.rowptr, "col": cc(g.rowptr, g.col, N)}

    @staticmethod
    def setup(t):
        return lambda: [t.dev.edge_candidates(_adj(t), 12345, 100, 200000)[1]]


def _select_args(t):
    return (t.ptr(t.row_map), t.ptr(t.col_map), int(t.host["n_out"][0]), int(t.host["n_out"][1]), None, 0, 1, 1 << 62, 5, 0, 0)


class _Select:
    """columns renumbered without every fifth, self loops and a hashed quarter of the entries dropped; the rows keep three in four and
    land on EVEN output rows, so that every other output row has no source row: its length is the zero the call's own memset wrote"""
    @staticmethod
    def host(d):
        g = graph()
        keep = np.arange(N) % 5 != 0
        cmap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        rows = np.arange(N) % 4 != 0
        rmap = np.where(rows, 2 * (np.cumsum(rows) - 1), -1).astype(np.int32)
        return {"rowptr": g.rowptr, "col": g.col, "val": g.val, "col_map": cmap, "row_map": rmap,
                "n_out": np.array([2 * rows.sum(), keep.sum()], dtype=np.int64)}


@case("sgl_csr_select_rowptr", "syncs", widths=(None,),
      doc=("header", "It allocates O(n_rows_out) scratch, frees it on return and so synchronises the DEVICE, like sgl_coo_to_csr"), waits="device")
class _(_Select):
    @staticmethod
    def host(d):
        h, g = _Select.host(d), graph()
        h["col"] = cc(g.rowptr, g.col, N)
        return h

    @staticmethod
    def setup(t):
        g = graph()
        o = t.out(int(t.host["n_out"][0]) + 1, dtype=t.torch.int64)

        def call():
            total = ctypes.c_int64(-1)
            t.call("sgl_csr_select_rowptr", t.ptr(t.rowptr), t.ptr(t.col), N, N, g.nnz, *_select_args(t), t.ptr(o), ctypes.byref(total))
            return [o, t.torch.tensor([total.value], dtype=t.torch.int64)]
        return call


@case("sgl_csr_select_fill", widths=(None,))
class _(_Select):
    """the row pointers of the result come from a first call in setup, on ready structure arrays: only the values are delayed (a
    decoy structure under the real row pointers would not be the pair of calls the header describes)"""
    @staticmethod
    def host(d):
        h = _Select.host(d)
        h["val"] = fl(h["val"])
        return h

    @staticmethod
    def setup(t):
        g = graph()
        rowptr_out = t.torch.empty(int(t.host["n_out"][0]) + 1, dtype=t.torch.int64, device=t.device)
        total = ctypes.c_int64(-1)
        t.call("sgl_csr_select_rowptr", t.ptr(t.rowptr), t.ptr(t.col), N, N, g.nnz, *_select_args(t), t.ptr(rowptr_out), ctypes.byref(total))
        m = total.value
        assert 0 < m < g.nnz
        col, val, pos = t.out(m, dtype=t.torch.int32), t.out(m), t.out(m, dtype=t.torch.int64)

        def call():
            t.call("sgl_csr_select_fill", t.ptr(t.rowptr), t.ptr(t.col), t.ptr(t.val), N, N, g.nnz, *_select_args(t), t.ptr(rowptr_out),
                   t.ptr(col), t.ptr(val), t.ptr(pos))
            return [col, val, pos]
        return call


class _Merge:
    @staticmethod
    def host(d):
        a, b = graph(), graph(11, 2)
        return {"a_rowptr": a.rowptr, "a_col": a.col, "a_val": a.val, "b_rowptr": b.rowptr, "b_col": b.col, "b_val": b.val}


@case("sgl_csr_merge_rowptr", "syncs", widths=(None,),
      doc=("header", "O(n_rows) scratch, freed on return: synchronises the DEVICE"), waits="device")
class _(_Merge):
    @staticmethod
    def host(d):
        h, a = _Merge.host(d), graph()
        h["a_col"] = cc(a.rowptr, a.col, N)
        return h

    @staticmethod
    def setup(t):
        a, b = graph(), graph(11, 2)
        o = t.out(N + 1, dtype=t.torch.int64)

        def call():
            total = ctypes.c_int64(-1)
            t.call("sgl_csr_merge_rowptr", t.ptr(t.a_rowptr), t.ptr(t.a_col), a.nnz, t.ptr(t.b_rowptr), t.ptr(t.b_col), b.nnz, N, N, 0, t.ptr(o),
                   ctypes.byref(total))
            return [o, t.torch.tensor([total.value], dtype=t.torch.int64)]
        return call


@case("sgl_csr_merge_fill", widths=(None,))
class _(_Merge):
    """as sgl_csr_select_fill: the row pointers come from setup, both value arrays are delayed"""
    @staticmethod
    def host(d):
        h = _Merge.host(d)
        h["a_val"], h["b_val"] = fl(h["a_val"]), fl(h["b_val"])
        return h

    @staticmethod
    def setup(t):
        a, b = graph(), graph(11, 2)
        rowptr_out = t.torch.empty(N + 1, dtype=t.torch.int64, device=t.device)
        total = ctypes.c_int64(-1)
        t.call("sgl_csr_merge_rowptr", t.ptr(t.a_rowptr), t.ptr(t.a_col), a.nnz, t.ptr(t.b_rowptr), t.ptr(t.b_col), b.nnz, N, N, 0,
               t.ptr(rowptr_out), ctypes.byref(total))
        m = total.value
        assert max(a.nnz, b.nnz) < m < a.nnz + b.nnz
        col, val, pa, pb = t.out(m, dtype=t.torch.int32), t.out(m), t.out(m, dtype=t.torch.int64), t.out(m, dtype=t.torch.int64)

        def call():
            t.call("sgl_csr_merge_fill", t.ptr(t.a_rowptr), t.ptr(t.a_col), t.ptr(t.a_val), a.nnz, t.ptr(t.b_rowptr), t.ptr(t.b_col),
                   t.ptr(t.b_val), b.nnz, N, N, t.lib.SGL_MERGE_SUM, 0, t.ptr(rowptr_out), t.ptr(col), t.ptr(val), t.ptr(pa), t.ptr(pb))
            return [col, val, pa, pb]
        return call


@case("sgl_coo_to_csr", "syncs", widths=(None,), doc=("header", "Synchronises `stream`; the temporaries are freed on return, so the call synchronises the DEVICE"), waits="device")
class _:
    @staticmethod
    def host(d):
        r, c, v = coo_list()
        return {"row": ix(r, N, 1), "col": ix(c, N, 2), "val": fl(v)}

    @staticmethod
    def setup(t):
        nnz = t.row.numel()
        rowptr, col, val = t.out(N + 1, dtype=t.torch.int64), t.out(nnz, dtype=t.torch.int32), t.out(nnz)

        def call():
            m = ctypes.c_int64(-1)
            t.call("sgl_coo_to_csr", N, N, nnz, t.ptr(t.row), t.ptr(t.col), t.ptr(t.val), t.ptr(rowptr), t.ptr(col), t.ptr(val), ctypes.byref(m))
            return [rowptr, col[:m.value], val[:m.value], t.torch.tensor([m.value], dtype=t.torch.int64)]
        return call

    @staticmethod
    def oracle(h):
        a = sp.coo_matrix((np.nan_to_num(h["val"].astype(np.float64), nan=1e9), (h["row"], h["col"])), shape=(N, N)).toarray()
        return a


@case("sgl_reorder_community", "syncs", via="reorder.community_order", widths=(None,),
      doc=("header", "Synchronises the stream; its temporaries are freed on return, so it synchronises the DEVICE"), waits="device")
class _:
    """two rounds of label propagation and the sort, on the structure alone: the columns are delayed"""
    @staticmethod
    def host(d):
        g = graph()
        return {"rowptr": g.rowptr, "col": cc(g.rowptr, g.col, N)}

    @staticmethod
    def setup(t):
        from sgl_amd import reorder
        return lambda: [reorder.community_order(t.rowptr, t.col, N, rounds=2)[0]]


@case("sgl_reorder_lpa_round", widths=(None,))
class _:
    """with a counter word of the caller's the call has nothing to free and does not wait"""
    @staticmethod
    def host(d):
        g = graph()
        labels = ((np.arange(N, dtype=np.int64) * 7) % 97).astype(np.int32)
        return {"rowptr": g.rowptr, "col": g.col, "labels": ix(labels, N, 13), "zero": np.zeros(1, dtype=np.int64)}

    @staticmethod
    def setup(t):
        o, moved = t.out(N, dtype=t.torch.int32), t.inout(t.zero)

        def call():
            t.call("sgl_reorder_lpa_round", t.ptr(t.rowptr), t.ptr(t.col), N, 0, N, t.ptr(t.labels), t.ptr(o), 1, 0, t.ptr(moved))
            return [o, moved]
        return call


@case("sgl_csr_permute_rows", "syncs", via="device.permute_rows", widths=(None,),
      doc=("header", "The temporaries are freed on return: this call synchronises the DEVICE"), waits="device")
class _:
    @staticmethod
    def host(d):
        g = graph()
        perm = np.random.default_rng(23).permutation(N).astype(np.int32)
        return {"rowptr": g.rowptr, "col": g.col, "val": fl(g.val), "perm": ix(perm, N, 9)}

    @staticmethod
    def setup(t):
        return lambda: list(t.dev.permute_rows(t.rowptr, t.col, t.val, t.perm))


# ---- normalisation ---------------------------------------------------------------------------------------------------------------------
def _norm_host():
    g = graph()
    return {"rowptr": g.rowptr, "col": g.col, "val": fl(g.val)}


def _prepare_case(entry, row0, doc):
    """sgl_norm_prepare / sgl_norm_block_prepare: the count of rows without a stored diagonal comes back through the host"""
    class _:
        @staticmethod
        def host(d):
            g = graph()
            return {"rowptr": g.rowptr, "col": cc(g.rowptr, g.col, N)}

        @staticmethod
        def setup(t):
            g = graph()

            def call():
                m = ctypes.c_int64(-1)
                t.call(entry, N, *row0, g.nnz, t.ptr(t.rowptr), t.ptr(t.col), ctypes.byref(m))
                return [t.torch.tensor([m.value], dtype=t.torch.int64)]
            return call

        @staticmethod
        def oracle(h):
            g = graph()
            return np.array([g.nnz + missing_diagonal(g._replace(col=h["col"]))])
    return case(entry, "syncs", widths=(None,), doc=doc, waits="device")(_)


_EXECUTE_DOC = ("header", "sgl_norm_prepare, sgl_norm_execute and sgl_norm_execute_lr free their temporaries on return: each of them synchronises the DEVICE")
_BUILD_DOC = ("header", "sgl_norm_block_prepare, sgl_norm_block_build and sgl_norm_build_symcheck free their temporaries on return: each of them synchronises the DEVICE")
_prepare_case("sgl_norm_prepare", (), _EXECUTE_DOC)
_prepare_case("sgl_norm_block_prepare", (0,), _BUILD_DOC)


def _norm_outputs(t, m, v32=True):
    return (t.out(N + 1, dtype=t.torch.int64), t.out(m, dtype=t.torch.int32)) + ((t.out(m),) if v32 else ()) + (t.out(m, dtype=t.torch.float64),)


@case("sgl_norm_execute", "syncs", widths=(None,), doc=_EXECUTE_DOC, waits="device")
class _:
    host = staticmethod(lambda d: _norm_host())

    @staticmethod
    def setup(t):
        g = graph()
        m = g.nnz + missing_diagonal(g)
        o = _norm_outputs(t, m)

        def call():
            t.call("sgl_norm_execute", N, g.nnz, t.ptr(t.rowptr), t.ptr(t.col), t.ptr(t.val), 0.5, 1, 0.15, m, *[t.ptr(q) for q in o])
            return list(o)
        return call


@case("sgl_norm_execute_lr", "syncs", widths=(None,), doc=_EXECUTE_DOC, waits="device")
class _:
    @staticmethod
    def host(d):
        h = _norm_host()
        rng = np.random.default_rng(41)
        h.update(left=rng.random(N) + 0.5, right=rng.random(N) + 0.5)
        return h

    @staticmethod
    def setup(t):
        g = graph()
        m = g.nnz + missing_diagonal(g)
        o = _norm_outputs(t, m)

        def call():
            t.call("sgl_norm_execute_lr", N, g.nnz, t.ptr(t.rowptr), t.ptr(t.col), t.ptr(t.val), t.ptr(t.left), t.ptr(t.right), 0, 0.0, m,
                   *[t.ptr(q) for q in o])
            return list(o)
        return call


@case("sgl_norm_degrees", widths=(None,))
class _:
    host = staticmethod(lambda d: _norm_host())

    @staticmethod
    def setup(t):
        o = t.out(N, dtype=t.torch.float64)

        def call():
            t.call("sgl_norm_degrees", N, 0, t.ptr(t.rowptr), t.ptr(t.col), t.ptr(t.val), t.ptr(o))
            return [o]
        return call


@case("sgl_norm_block_build", "syncs", widths=(None,), doc=_BUILD_DOC, waits="device")
class _:
    host = staticmethod(lambda d: _norm_host())

    @staticmethod
    def setup(t):
        g = graph()
        m = g.nnz + missing_diagonal(g)
        o = _norm_outputs(t, m, v32=False) + (t.out(N, dtype=t.torch.float64),)

        def call():
            t.call("sgl_norm_block_build", N, 0, g.nnz, t.ptr(t.rowptr), t.ptr(t.col), t.ptr(t.val), m, *[t.ptr(q) for q in o])
            return list(o)
        return call


@case("sgl_norm_build_symcheck", "syncs", widths=(None,), doc=_BUILD_DOC, waits="device")
class _:
    @staticmethod
    def host(d):
        h = _norm_host()
        h["zero"] = np.zeros(1, dtype=np.int64)
        return h

    @staticmethod
    def setup(t):
        g = graph()
        m = g.nnz + missing_diagonal(g)
        o = _norm_outputs(t, m, v32=False) + (t.out(N, dtype=t.torch.float64), t.inout(t.zero))

        def call():
            t.call("sgl_norm_build_symcheck", N, g.nnz, t.ptr(t.rowptr), t.ptr(t.col), t.ptr(t.val), m, *[t.ptr(q) for q in o])
            return list(o)
        return call


def _block_host(name="val64"):
    """the pattern of A + I (every row stores its diagonal), float64 values with few significant bits"""
    g = graph(7, 1)
    h = {"rowptr": g.rowptr, "col": g.col, name: fl(g.val.astype(np.float64)), "diag": diag_positions(g)}
    rng = np.random.default_rng(43)
    h.update(left=rng.random(N) + 0.5, right=rng.random(N) + 0.5)
    return h


@case("sgl_norm_block_colsum", widths=(None,))
class _:
    """float64 atomics: the real values are small integers, so every order of the additions gives the same bits"""
    @staticmethod
    def host(d):
        g = graph(7, 1)
        v = ((np.arange(g.nnz) % 5) + 1).astype(np.float64)
        return {"col": g.col, "val64": fl(v), "zero": np.zeros(N, dtype=np.float64)}

    @staticmethod
    def setup(t):
        o = t.inout(t.zero)

        def call():
            t.call("sgl_norm_block_colsum", N, t.col.numel(), t.ptr(t.col), t.ptr(t.val64), t.ptr(o))
            return [o]
        return call

    @staticmethod
    def oracle(h):
        return np.bincount(h["col"], weights=h["val64"], minlength=N)


@case("sgl_norm_block_scale", widths=(None,))
class _:
    host = staticmethod(lambda d: _block_host())

    @staticmethod
    def setup(t):
        m = t.col.numel()
        o = (t.out(m), t.out(m, dtype=t.torch.float64))

        def call():
            t.call("sgl_norm_block_scale", N, 0, t.ptr(t.rowptr), t.ptr(t.col), t.ptr(t.val64), t.ptr(t.left), t.ptr(t.right), 1, 0.15,
                   t.ptr(o[0]), t.ptr(o[1]))
            return list(o)
        return call


@case("sgl_norm_block_mix", widths=(None,))
class _:
    host = staticmethod(lambda d: _block_host("hat64"))

    @staticmethod
    def setup(t):
        m = t.col.numel()
        o = (t.out(m), t.out(m, dtype=t.torch.float64))

        def call():
            t.call("sgl_norm_block_mix", N, 0, t.ptr(t.rowptr), t.ptr(t.col), t.ptr(t.hat64), 0.15, t.ptr(o[0]), t.ptr(o[1]))
            return list(o)
        return call


@case("sgl_norm_block_mix_at", widths=(None,))
class _:
    host = staticmethod(lambda d: _block_host("hat64"))

    @staticmethod
    def setup(t):
        m = t.col.numel()
        o = (t.out(m), t.out(m, dtype=t.torch.float64))

        def call():
            t.call("sgl_norm_block_mix_at", m, N, t.ptr(t.hat64), t.ptr(t.diag), 0.15, t.ptr(o[0]), t.ptr(o[1]))
            return list(o)
        return call


@case("sgl_norm_block_diag_positions", widths=(None,))
class _:
    @staticmethod
    def host(d):
        g = graph()
        return {"rowptr": g.rowptr, "col": cc(g.rowptr, g.col, N)}

    @staticmethod
    def setup(t):
        o = t.out(N, dtype=t.torch.int64)

        def call():
            t.call("sgl_norm_block_diag_positions", N, 0, t.ptr(t.rowptr), t.ptr(t.col), t.ptr(o))
            return [o]
        return call

    @staticmethod
    def oracle(h):
        return diag_positions(graph()._replace(col=h["col"]))


@case("sgl_norm_degree_powers", widths=(None,))
class _:
    @staticmethod
    def host(d):
        return {"deg": fl(np.random.default_rng(47).random(N) * 20 + 1)}

    @staticmethod
    def setup(t):
        o = (t.out(N, dtype=t.torch.float64), t.out(N, dtype=t.torch.float64))

        def call():
            t.call("sgl_norm_degree_powers", N, t.ptr(t.deg), 0.5, t.ptr(o[0]), t.ptr(o[1]))
            return list(o)
        return call


# ---- include/sgl_probe.h: the synthetic-workload generators -------------------------------------------------------------------------------
@case("sgl_synth_degrees", via="ctypes (probe_lib)", widths=(None,))
class _:
    @staticmethod
    def host(d):
        table = np.sort(np.random.default_rng(51).integers(1, 60, 8192)).astype(np.int32)
        return {"table": ix(table, 60, 4096)}

    @staticmethod
    def setup(t):
        o = t.out(N, dtype=t.torch.int64)

        def call():
            t.probe("sgl_synth_degrees", ctypes.c_uint64(99), 5, N, t.ptr(t.table), t.ptr(o))
            return [o]
        return call


@case("sgl_synth_fill", via="ctypes (probe_lib)", widths=(None,), inputless=True)
class _:
    """its only device input is the row pointer array, which says where every row is written: it stays ready, and the outputs'
    sentinel, written on S behind the delay, is what a launch on another stream would be lost under"""
    @staticmethod
    def host(d):
        return {"rowptr": graph().rowptr}

    @staticmethod
    def setup(t):
        nnz = graph().nnz
        col, val = t.out(nnz, dtype=t.torch.int32), t.out(nnz)

        def call():
            t.probe("sgl_synth_fill", ctypes.c_uint64(99), 5, N, 4 * N, t.ptr(t.rowptr), t.ptr(col), t.ptr(val))
            return [col, val]
        return call


@case("sgl_synth_features", via="ctypes (probe_lib)", inputless=True)
class _:
    """no device input at all: see sgl_synth_fill"""
    @staticmethod
    def host(d):
        return {"width": np.array([d], dtype=np.int64)}

    @staticmethod
    def setup(t):
        d = int(t.host["width"][0])
        o = t.out_rows(N, d)
        parent = t.dev.padded_parent(o)

        def call():
            t.probe("sgl_synth_features", ctypes.c_uint64(99), 5, N, d, parent.stride(0), t.ptr(parent))
            return [o]
        return call


# ---- wrapper-level flows: the feature matrix (or, where there is none, the value array) delayed ------------------------------------------
# Same protocol, same machinery; these are not header functions, so they live in FLOWS, outside the completeness check.  Their
# wrappers read sizes, fingerprints and flags through the host, so only the values decide (class "syncs" without a quote to find).
FLOWS = {}
FLOW_WIDTH = 100


def flow(name, inputless=False):
    def deco(cls):
        assert name not in FLOWS
        FLOWS[name] = Case(name, "syncs", "wrapper", (FLOW_WIDTH,), cls.host, cls.setup, None, inputless, None, None)
        return cls
    return deco


class forced_delta:
    """config.delta_propagate for the duration of a call: True also drops the size threshold, so that a matrix this small qualifies"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from sgl_amd import config
        self.saved = (config.delta_propagate, config.delta_propagate_min_mb)
        config.delta_propagate, config.delta_propagate_min_mb = bool(self.on), 0.0 if self.on else self.saved[1]

    def __exit__(self, *exc):
        from sgl_amd import config
        config.delta_propagate, config.delta_propagate_min_mb = self.saved


def scipy_graph():
    g = graph()
    return sp.csr_matrix((g.val.copy(), g.col.copy(), g.rowptr.copy()), shape=(N, N))


def _propagate_flow(op_name, hop_dtype, delta, second):
    """GraphOp.propagate over the scipy graph with X delayed; second: a first call with other values in the last four columns ran in
    setup, so that with delta_propagate forced on the call under test takes the column-delta path (asserted).  Hop 0 is the
    caller's own matrix (the delayed buffer, for float32) and is left out of the outputs."""
    class _:
        @staticmethod
        def host(d):
            x = feats(d)[0]
            h = {"x": fl(x)}
            if second:
                first = x.copy()
                first[:, -4:] += np.float32(1)
                h["x_first"] = first
            return h

        @staticmethod
        def setup(t):
            from sgl_amd.operators.graph_op import LaplacianGraphOp, PprGraphOp
            adj = scipy_graph()
            op = LaplacianGraphOp(3, r=0.5, hop_dtype=hop_dtype) if op_name == "laplacian" else PprGraphOp(3, r=0.5, alpha=0.15,
                                                                                                         hop_dtype=hop_dtype)
            t.keep = [op, adj]
            if second:
                with forced_delta(delta):
                    t.keep.append(op.propagate(adj, t.x_first))

            def call():
                with forced_delta(delta):
                    hops = op.propagate(adj, t.x)
                if delta and second and hop_dtype == "float32" and t.expect_real:
                    assert op.delta_info is not None and op.delta_info["columns_propagated"] == (FLOW_WIDTH - 4, FLOW_WIDTH), op.delta_info
                assert len(hops) == 4
                return list(hops[1:])
            return call
    return flow(f"propagate-{op_name}-{hop_dtype}-{'delta' if delta else 'full'}-{'second' if second else 'first'}")(_)


for _op in ("laplacian", "ppr"):
    for _dtype, _delta in (("float32", False), ("float32", True), ("bfloat16", False)):
        for _second in (False, True):
            _propagate_flow(_op, _dtype, _delta, _second)


def _aggregate_flow(kind, bf16):
    class _(_HopsBf16 if bf16 else _Hops):
        @staticmethod
        def setup(t):
            from sgl_amd.operators import message_op as mo
            op = mo.OverSmoothDistanceWeightedOp() if kind == "nafs" else getattr(mo, kind.capitalize() + "MessageOp")(0, H)
            hops = _Hops.hops(t)
            return lambda: [op.aggregate(hops)]
    return flow(f"aggregate-{kind}-{'bfloat16' if bf16 else 'float32'}")(_)


def _weighted_flow(kind, arg, bf16):
    """SimpleWeightedMessageOp: no learnable state, its weights are fixed at construction"""
    class _(_HopsBf16 if bf16 else _Hops):
        @staticmethod
        def setup(t):
            from sgl_amd.operators.message_op import SimpleWeightedMessageOp
            op = SimpleWeightedMessageOp(0, H, kind, arg)
            hops = _Hops.hops(t)
            op.aggregate(hops)                    # the fixed weights move to the device at their first use: here, not under the delay
            return lambda: [op.aggregate(hops)]
    return flow(f"aggregate-weighted-{kind}-{'bfloat16' if bf16 else 'float32'}")(_)


# every stateless MessageOp but LastMessageOp, which returns its last input untouched (no kernel, no copy: there is nothing to
# order).  The learnable ones (LearnableWeighted, IterateLearnableWeighted, ProjectedConcat) hold parameters; the entry points under
# them are in the table.
for _kind in ("concat", "sum", "mean", "max", "min", "nafs"):
    for _bf16 in (False, True):
        _aggregate_flow(_kind, _bf16)
for _bf16 in (False, True):
    _weighted_flow("alpha", 0.3, _bf16)
    _weighted_flow("hand_crafted", [0.5, 0.25, 0.125, 0.125], _bf16)


class _Transform:
    @staticmethod
    def host(d):
        g = graph()
        rng = np.random.default_rng(61)
        return {"rowptr": g.rowptr, "col": g.col, "val": fl(g.val), "x": fl(feats(d)[0]),
                "node_mask": rng.random(N) < 0.6, "edge_mask": rng.random(g.nnz) < 0.7}

    @staticmethod
    def adj(t):
        from sgl_amd.io import DeviceAdjacency
        return DeviceAdjacency(t.rowptr, t.col, t.val, (N, N))

    @staticmethod
    def parts(a):
        return [a.rowptr, a.col, a.val]


@flow("transforms.get_subgraph")
class _(_Transform):
    @staticmethod
    def setup(t):
        from sgl_amd import transforms

        def call():
            sub = transforms.get_subgraph(_Transform.adj(t), t.node_mask, x=t.x)
            return _Transform.parts(sub.adj) + [sub.x, sub.node_ids]
        return call


@flow("transforms.drop_edges")
class _(_Transform):
    @staticmethod
    def setup(t):
        from sgl_amd import transforms
        return lambda: _Transform.parts(transforms.drop_edges(_Transform.adj(t), t.edge_mask, force_undirected=True))


@flow("transforms.to_undirected")
class _(_Transform):
    @staticmethod
    def setup(t):
        from sgl_amd import transforms
        return lambda: _Transform.parts(transforms.to_undirected(_Transform.adj(t)))


@flow("mask_test_edges")
class _:
    """the split follows from the structure: the columns are delayed as well as the values"""
    @staticmethod
    def host(d):
        g = graph()
        return {"rowptr": g.rowptr, "col": cc(g.rowptr, g.col, N), "val": fl(g.val)}

    @staticmethod
    def setup(t):
        from sgl_amd.tricks.link_prediction import mask_test_edges

        def call():
            split = mask_test_edges(_Transform.adj(t), seed=3, device=t.device)
            return _Transform.parts(split[0]) + list(split[1:])
        return call


@flow("kmeans")
class _:
    @staticmethod
    def host(d):
        return {"x": fl(feats(d)[0]), "centres": feats(d, 6)[1][:K_CENTRES].copy()}

    @staticmethod
    def setup(t):
        from sgl_amd.tricks.clustering import kmeans

        def call():
            r = kmeans(t.x, K_CENTRES, max_iter=3, init=t.centres.contiguous())
            return [r.labels, r.centres]
        return call


def _with_backward(t, name, loss_of):
    """forward and backward of a loss over the delayed matrix: (loss, gradient)"""
    def call():
        z = getattr(t, name).detach().requires_grad_()
        loss = loss_of(z)
        loss.backward()
        return [loss.detach().reshape(1), z.grad]
    return call


def _edge_bce_flow(name, fused):
    class _:
        @staticmethod
        def host(d):
            e = edge_list()
            return {"z": fl(feats(d)[0] / np.float32(8)), "edges": e, "labels": (np.arange(len(e)) % 3 == 0).astype(np.float32)}

        @staticmethod
        def setup(t):
            from sgl_amd.tricks.link_prediction import EdgePlan, edge_bce_loss
            plan = EdgePlan(t.edges, t.labels, N, max_piece=32, device=t.device)
            assert plan.n_partial >= 2
            return _with_backward(t, "z", lambda z: edge_bce_loss(z, plan, fused=fused))
    return flow(name)(_)


_edge_bce_flow("edge_bce_loss", False)
_edge_bce_flow("edge_bce_loss-fused", True)


@flow("cluster_loss")
class _:
    @staticmethod
    def host(d):
        y = (np.arange(N, dtype=np.int64) * 3) % K_CENTRES
        return {"x": fl(feats(d)[0]), "centres": feats(d, 6)[1][:K_CENTRES].copy(), "labels": y}

    @staticmethod
    def setup(t):
        from sgl_amd.tricks.clustering import cluster_loss
        return _with_backward(t, "x", lambda x: cluster_loss(x, t.labels, t.centres))


@flow("cross_entropy")
class _:
    @staticmethod
    def host(d):
        return {"z": fl(feats(d)[0]), "labels": (np.arange(N, dtype=np.int64) * 5) % d}

    @staticmethod
    def setup(t):
        from sgl_amd.tricks.classification import cross_entropy
        return _with_backward(t, "z", lambda z: cross_entropy(z, t.labels, fused=True))


# ---- header parsing (test_stream_cpu.py) ---------------------------------------------------------------------------------------------------
_DECL = re.compile(r"\b(?:int|void|int64_t)\s+(\w+)\s*\(([^;{}]*?)\)\s*;", re.S)


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def stream_functions(header_text):
    """the names of the functions declared in a header whose last parameter is `void *stream`"""
    return [m.group(1) for m in _DECL.finditer(strip_comments(header_text)) if re.search(r"void\s*\*\s*stream\s*$", m.group(2).strip())]


def normalised(text):
    """comment text with the line decoration and the line breaks taken out"""
    return re.sub(r"\s+", " ", re.sub(r"^\s*\*\s?", " ", text, flags=re.M).replace("/*", " ").replace("*/", " "))


# ---- the GPU side (imports torch when called) ------------------------------------------------------------------------------------------
_COMM = []


def one_rank_communicator():
    """a one-rank communicator of the real librccl, created once per process (pytest.skip without the library)"""
    import pytest
    if _COMM:
        return _COMM[0]

    class UniqueId(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_char * 128)]
    try:
        rccl = ctypes.CDLL("librccl.so.1", mode=ctypes.RTLD_GLOBAL)
    except OSError:
        pytest.skip("no librccl.so.1 on this box")
    uid = UniqueId()
    assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
    comm = ctypes.c_void_p()
    rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UniqueId, ctypes.c_int]
    assert rccl.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    rccl.ncclCommDestroy.argtypes = [ctypes.c_void_p]
    atexit.register(rccl.ncclCommDestroy, comm)
    _COMM.append(comm)
    return comm


_CAL = {}


def calibrate(device):
    """cycles of torch.cuda._sleep per millisecond on this device, measured once per process with two events"""
    import torch
    if "cycles_per_ms" not in _CAL:
        cycles = 1 << 20
        for _ in range(8):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0:
                break
            cycles *= 4
        _CAL.update(cycles_per_ms=cycles / ms, calibration_cycles=cycles, calibration_ms=ms)
    return _CAL["cycles_per_ms"]


def delay(stream, ms):
    """a bounded busy-wait of about `ms` milliseconds queued on `stream`"""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(calibrate(stream.device) * ms))


_SIDE = {}


def runs_ahead(victim, delayed, ms=3.0):
    """does a kernel queued on `victim` finish while `delayed` is busy-waiting?  With fewer hardware queues than streams
    (GPU_MAX_HW_QUEUES) two streams can share one, and work on either then runs in the order it was queued on BOTH: nothing wrong,
    but a launch that went to `victim` by mistake would wait behind the delay like a correct one, and the test would be blind."""
    import torch
    torch.cuda.synchronize()
    behind, done = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(delayed):
        delay(delayed, ms)
        behind.record(delayed)
    with torch.cuda.stream(victim):
        torch.zeros(64, device=delayed.device).add_(1)
        done.record(victim)
    done.synchronize()
    ahead = not behind.query()
    delayed.synchronize()
    return ahead


def independent_stream(device, others=(), key="S"):
    """A non-blocking side stream (torch creates them so) that is verified NOT to share a hardware queue with the default stream
    nor with any of `others`: work queued on those runs ahead of a delay queued on it, and the other way round.  Found once per
    (device, key) among fresh torch.cuda.Stream()s and kept."""
    import torch
    if (str(device), key) not in _SIDE:
        rivals = [torch.cuda.default_stream(device)] + list(others)
        for _ in range(64):
            cand = torch.cuda.Stream(device=device)
            if all(runs_ahead(r, cand) and runs_ahead(cand, r) for r in rivals):
                _SIDE[(str(device), key)] = cand
                break
        else:
            raise RuntimeError("no side stream with a hardware queue of its own among 64 fresh streams")
    return _SIDE[(str(device), key)]


class Env:
    """what a case's setup sees: `t.<name>` = the device tensor of every host input (a delayed one: the buffer whose content the
    protocol swaps), output allocators, the call paths"""

    def __init__(self, host, which, device):
        import torch
        from sgl_amd import _lib
        from sgl_amd import device as dev
        self.torch, self.lib, self.dev, self.device, self.host = torch, _lib, dev, device, host
        self.ptr = _lib.ptr
        self.delayed, self.outputs, self.inouts = {}, [], []
        self.expect_real = which == "real"           # the call sees the real inputs (the protocol sets it: they arrive behind the delay)
        for name, a in host.items():
            if isinstance(a, Delayed):
                real, decoy = self.upload(a.real), self.upload(a.decoy)
                buf = self.upload(a.real if which == "real" else a.decoy)
                self.delayed[name] = (buf, real, decoy)
                setattr(self, name, buf)
            else:
                setattr(self, name, self.upload(a))

    def upload(self, a):
        torch = self.torch
        if a.dtype == np.uint16:                                               # bfloat16 bit patterns
            src = torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)
        else:
            src = torch.from_numpy(a)
        if a.ndim == 2 and a.dtype in (np.float32, np.uint16):
            out = self.dev.alloc_rows(a.shape[0], a.shape[1], self.device, dtype=src.dtype)
            out.copy_(src)
            return out
        return src.to(self.device)

    def call(self, name, *args, raw=False):
        """the product's call path: the current stream is appended there"""
        return self.dev._call(self.device, name, *args, raw=raw)

    def probe(self, name, *args):
        with self.torch.cuda.device(self.device):
            self.lib.check_probe(getattr(self.lib.probe_lib(), name)(*args, self.lib.current_stream_ptr()), name)

    @staticmethod
    def poison(o):
        o.fill_(-77 if not o.dtype.is_floating_point else -12345.5)

    def out(self, *shape, dtype=None, poison=True):
        o = self.torch.empty(shape, dtype=dtype or self.torch.float32, device=self.device)
        self.poison(o)
        if poison:
            self.outputs.append(o)
        return o

    def out_rows(self, n, d, bf16=False):
        o = self.dev.alloc_rows(n, d, self.device, dtype=self.torch.bfloat16 if bf16 else self.torch.float32)
        self.poison(o)
        self.outputs.append(o)
        return o

    def inout(self, init):
        """an array the call reads AND writes (a running aggregate, a zeroed counter): a fresh copy of `init` per run, put back on S
        behind the delay like the sentinel of an output"""
        o = init.clone()
        self.inouts.append((o, init))
        return o


def snapshot(host_tensors):
    """the bits of a list of host tensors: (dtype, shape, bytes) each"""
    import torch
    out = []
    for h in host_tensors:
        h = h.contiguous()
        out.append((str(h.dtype), tuple(h.shape), h.reshape(-1).view(torch.uint8).numpy().tobytes() if h.numel() else b""))
    return out


def to_host(outs, pinned):
    """the outputs as host tensors; device tensors travel on the current stream, into pinned memory when asked (non-blocking)"""
    import torch
    host = []
    for o in outs:
        if not o.is_cuda:
            host.append(o.clone())
        elif pinned:
            h = torch.empty(o.shape, dtype=o.dtype, pin_memory=True)
            h.copy_(o, non_blocking=True)
            host.append(h)
        else:
            host.append(o.cpu())
    return host


def plain_run(c, d, device, which="real", before=False):
    """(bits of the outputs, host seconds of the call) of a run on the default stream with ready inputs; before=True: also the
    bits of the sentinel-filled outputs the case allocated in setup, as they were before the call"""
    import torch
    t = Env(c.host(d), which, device)
    call = c.setup(t)
    torch.cuda.synchronize()
    poisoned = snapshot(to_host(t.outputs, pinned=False)) if before else None
    t0 = time.perf_counter()
    outs = call()
    dt = time.perf_counter() - t0
    bits = snapshot(to_host(outs, pinned=False))
    torch.cuda.synchronize()
    return (bits, dt, poisoned) if before else (bits, dt)


def run_behind_delay(c, d, device, delay_ms, want):
    """The protocol of the module docstring for case c at width d.  Returns a dict of what was observed: `pending_before` /
    `pending_after` (the event behind the real inputs had not completed just before / right after the call), `host_ms` of the call,
    `equal` (the host copy has want's bits)."""
    import torch
    t = Env(c.host(d), "decoy", device)
    t.expect_real = True
    call = c.setup(t)
    for o in t.outputs:
        t.poison(o)
    torch.cuda.synchronize()
    side = independent_stream(device)
    filled = torch.cuda.Event()
    with torch.cuda.stream(side):
        delay(side, delay_ms)
        for buf, real, _ in t.delayed.values():
            buf.copy_(real, non_blocking=True)
        for o in t.outputs:
            t.poison(o)
        for o, init in t.inouts:
            o.copy_(init, non_blocking=True)
        filled.record(side)
        pending_before = not filled.query()
        t0 = time.perf_counter()
        outs = call()
        host_ms = (time.perf_counter() - t0) * 1e3
        pending_after = not filled.query()
        for buf, _, decoy in t.delayed.values():
            buf.copy_(decoy, non_blocking=True)
        host = to_host(outs, pinned=True)
    side.synchronize()
    got = snapshot(host)
    return {"pending_before": pending_before, "pending_after": pending_after, "host_ms": host_ms, "equal": got == want,
            "first_difference": first_difference(got, want)}


def dirty_scratch(device, sizes=tuple(1 << k for k in range(12, 21))):
    """hipMalloc, fill with 0xFF and hipFree a few blocks (through the probe library's sgl_mem_alloc / sgl_mem_free): where the
    runtime hands freed memory out again as it is, the scratch arrays an entry point allocates next do not start out as zeros, and a
    memset of theirs that runs late -- or not at all -- is visible in the result"""
    import torch
    from sgl_amd import device as dev
    with torch.cuda.device(device):
        blocks = [dev.placed_empty((n // 4,), device, mode="default") for n in sizes for _ in range(4)]
        for b in blocks:
            b.view(torch.int32).fill_(-1)
        torch.cuda.synchronize()
        del blocks, b


def run_ahead_of_bystander(c, d, device, delay_ms, want):
    """Why this second run exists, at twice the table's GPU work: run_behind_delay cannot see an INITIALISER on the wrong stream.  A
    memset of library scratch queued on the null stream runs EARLY there (S is the delayed one), before the kernel that needs it --
    the right order by accident; `nullptr` for `st` in the memset of sgl_csr_select_rowptr passes that run.  Here the null stream is
    the late one, and dirty_scratch() sees to it that scratch which is not zeroed in time does not happen to be zero already: the
    same mutation fails.  It is also the only run that tells a wait for the stream from a wait for the device.

    The mirror image of run_behind_delay: the inputs are ready and the call runs on S, while the DEFAULT stream is the one that
    busy-waits for D.  Whatever the call put on the null stream -- the memset of a scratch array, a kernel, a copy -- then happens
    LATE: after the call's other work, after the outputs have travelled on S.  The host copy made on S has want's bits, and so has a
    second copy made once the default stream has drained (a late write lands there).  `pending_after`: the default stream was still
    busy when the call returned -- the call did not synchronise the DEVICE."""
    import torch
    t = Env(c.host(d), "real", device)
    call = c.setup(t)
    for o in t.outputs:
        t.poison(o)
    dirty_scratch(device)
    torch.cuda.synchronize()
    side, null = independent_stream(device), torch.cuda.default_stream(device)
    busy = torch.cuda.Event()
    delay(null, delay_ms)
    busy.record(null)
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        outs = call()
        host_ms = (time.perf_counter() - t0) * 1e3
        pending_after = not busy.query()
        host = to_host(outs, pinned=True)
    side.synchronize()
    got = snapshot(host)
    torch.cuda.synchronize()                 # the delay is over: only now a device-wide synchronisation
    later = snapshot(to_host(outs, pinned=False))
    return {"pending_after": pending_after, "host_ms": host_ms, "equal": got == want, "equal_later": later == want,
            "first_difference": first_difference(got, want) or first_difference(later, want)}


def first_difference(got, want):
    if got == want:
        return None
    if len(got) != len(want):
        return f"{len(got)} outputs, expected {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        if g[:2] != w[:2]:
            return f"output {k}: {g[:2]} instead of {w[:2]}"
        if g[2] != w[2]:
            a, b = np.frombuffer(g[2], dtype=np.uint8), np.frombuffer(w[2], dtype=np.uint8)
            bad = np.flatnonzero(a != b)
            return f"output {k} {w[:2]}: {len(bad)} of {len(a)} bytes differ, the first at byte {int(bad[0])}"
    return None

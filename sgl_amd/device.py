"""Thin Python layer over the C ABI (include/sgl_hip.h): device CSR handle, SpMM, aggregators.

torch is used for device memory, streams and autograd bookkeeping only; every computation
below is a hand-written HIP kernel in libsgl_hip.so.  There is no CPU fallback."""
import ctypes
import os
from ctypes import c_int64, c_void_p

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, current_stream_ptr, lib, ptr
from ._lib import leading_dim as _ld

__all__ = [
    "DeviceCSR", "default_long_row_nnz", "ChainGraph", "round_up", "row_pitch", "expected_lines", "alloc_rows", "upload_rows", "normalize_adj",
    "normalize_block", "degree_powers", "PreparedAdjacency", "PreparedBlock",
    "placed_empty", "MEM_MODES",
    "hop_reduce", "hop_concat", "hop_reduce_grad", "hop_concat_grad", "hop_lincomb", "hop_wsum1d", "hop_wsum2d", "hop_scores", "hop_scores2", "hop_gate", "gate_fusable", "nafs_aggregate", "nafs_prefix",
    "gather_rows", "edge_dot", "ensemble_combine",
]


def round_up(x, m):
    return (x + m - 1) // m * m


HOP_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
# hop aggregate kind -> (SGL_REDUCE_* code of the aggregator kernels, accumulate mode of the SpMM epilogue or None where it has none)
HOP_KINDS = {"sum": (_lib.SGL_REDUCE_SUM, 0), "mean": (_lib.SGL_REDUCE_MEAN, None), "wsum": (_lib.SGL_REDUCE_WSUM, 1),
             "max": (_lib.SGL_REDUCE_MAX, 2), "min": (_lib.SGL_REDUCE_MIN, 3)}


def hop_torch_dtype(dtype):
    """torch dtype of a hop storage dtype given as "float32" / "bfloat16" or as the torch dtype itself"""
    if isinstance(dtype, str):
        if dtype.strip().lower() not in HOP_DTYPES:
            raise ValueError(f"hop_dtype must be one of {sorted(HOP_DTYPES)}, not {dtype!r}")
        return HOP_DTYPES[dtype.strip().lower()]
    if dtype not in HOP_DTYPES.values():
        raise ValueError(f"hop matrices are stored as float32 or bfloat16, not {dtype}")
    return dtype


def _esize(dtype):
    return 2 if dtype == torch.bfloat16 else 4


# entry points whose last argument is not a stream
_NO_STREAM = frozenset({"sgl_csr_set_values", "sgl_csr_info", "sgl_csr_destroy", "sgl_chain_graph_create", "sgl_chain_graph_destroy",
                        "sgl_hop_colsum_scratch", "sgl_hop_wsum1d_bwd_scratch", "sgl_ensemble_combine_bwd_scratch"})


def _call(device, name, *args, raw=False):
    """One call of the library entry point `name` on `device` (None: whichever is current): the symbol is looked up on lib() when the
    call is made, the current stream of that device is appended for the entry points that take one, and the return code is checked
    under the same name.  raw=True hands the return value back unchecked (the scratch sizes; the two callers that branch on
    SGL_ERR_UNSUPPORTED).  Nothing here synchronises, allocates or touches a tensor: callers run under hipGraph capture."""
    with torch.cuda.device(device):
        if name not in _NO_STREAM:
            args += (current_stream_ptr(),)
        rc = getattr(lib(), name)(*args)
    if raw:
        return rc
    check(rc, name)


def _opt_ptr(t):
    return ptr(t) if t is not None else None


# ---- row layout: the three questions every launch asks about a [n, d] matrix.  Pure functions of shape, strides, storage offset,
# element size, base address and storage size (no is_cuda, no dtype test: those stay with the caller, like the column stride)
def pitch_vectored(t):
    """is the row stride, as torch reports it (for a single row too), a whole number of 16-byte vectors?"""
    return t.stride(0) % (16 // t.element_size()) == 0


def rows_vectored(t, single_row=False, width=None, room=False):
    """Are the rows of t 16-byte vectors -- base address and row pitch multiples of 16 bytes?  single_row: does a matrix of at most
    one row pass (its pitch is never stepped by)?  width: the columns the pitch has to cover (None: not asked; callers pass
    round_up(d, 4) when the kernel reads or writes the vector that straddles column d).  room: the storage must hold `width` columns
    of the LAST row too (that vector is read there as well)."""
    n = t.shape[0]
    if t.data_ptr() % 16:
        return False
    if n > 1:
        if not pitch_vectored(t) or (width is not None and t.stride(0) < width):
            return False
    elif not single_row:
        return False
    if room:
        have = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        return have >= (n - 1) * t.stride(0) * (n > 1) + width
    return True


def own_out_pad(ld, d):
    """The pad_cols of a float32 output WE allocated on a pitch of ld (alloc_rows) and hand to a gather kernel: the whole tail of the
    pitch while that is under 32 columns (every line of a row is then written whole), else up to the next 16-byte vector.  What
    lies beyond is zeroed by the caller."""
    return ld - d if ld - d < 32 else round_up(d, 4) - d


def expected_lines(ld, d, elem_size=4):
    """average number of 128-byte cache lines a row of d elements touches when rows are laid out at a pitch of ld elements of
    `elem_size` bytes (4: float32, the default; 2: bfloat16)"""
    import math
    step = math.gcd(ld * elem_size, 128)
    offs = range(0, 128, step)
    return sum((o + d * elem_size + 127) // 128 for o in offs) / len(offs)


def row_pitch(d, growth=1.25, elem_size=4):
    """Leading dimension (elements) for a hop matrix of width d; elem_size = 4 (float32 rows, the default) or 2 (bfloat16 rows).

    2-byte rows follow the same reasoning with 16-byte vectors of 8 elements and lines of 64: the pitch is a multiple of 8, rounded
    up to whole lines (or, for narrow rows, to a power of two) when that makes a gathered row touch measurably fewer lines within
    the growth cap -- d = 100 -> 128 (always exactly 2 lines; 104 would average 2.5; both measured, profiles/bf16_hop_dtype.json),
    d = 147 -> 152, d = 500 -> 512.  For float32 rows:

    Always a multiple of 4 floats (16-byte aligned rows -> 16-byte lane accesses).  The SpMM is bound by the number of
    128-byte lines it pulls through the fabric, so when rounding the pitch up to a whole number of lines
    (or, for narrow rows, to a power of two that never straddles a line) makes every gathered row touch measurably
    fewer lines, take it: d = 147 -> 160 floats (5 lines instead of 5.5 on average, +8 % memory), d = 500 -> 512,
    d = 12 -> 16; d = 100 stays 100 (always exactly 4 lines either way).  `growth` caps the memory overhead."""
    d = max(int(d), 1)
    if elem_size not in (2, 4):
        raise ValueError("row_pitch: elem_size must be 4 (float32) or 2 (bfloat16)")
    vec, line = 16 // elem_size, 128 // elem_size            # elements per 16-byte lane access / per 128-byte line
    ld4, ld32 = round_up(d, vec), round_up(d, line)
    cands = [(ld32, growth)]
    if d < line:
        p2 = vec
        while p2 < d:
            p2 *= 2
        cands.insert(0, (p2, max(growth, 1.34)))
    best, best_lines = ld4, expected_lines(ld4, d, elem_size)
    for ld, cap in cands:
        if ld != ld4 and ld <= cap * ld4 and expected_lines(ld, d, elem_size) <= 0.97 * best_lines:
            best, best_lines = ld, expected_lines(ld, d, elem_size)
    return best


def alloc_rows(n, d, device, zero_pad=True, dtype=torch.float32):
    """[n, d] view (float32 by default; torch.bfloat16 for bf16 hop storage) of a row-padded buffer (pitch = row_pitch(d) for the
    element size): every row starts 16-byte aligned, so the kernels use 16-byte lane accesses for any d, and rows are placed to
    touch as few cache lines as possible.  Pad columns are zero and stay zero under propagation."""
    ld = row_pitch(d, elem_size=_esize(dtype))
    buf = torch.empty((n, ld), dtype=dtype, device=device)
    if zero_pad and ld != d:
        buf[:, d:].zero_()
    return buf[:, :d] if ld != d else buf


def own_pad(t):
    """pad columns of an output WE allocated with alloc_rows (the tail of its pitch): what the *_padded_f32 entry points may write
    as zeros so that every line of a row is written whole; 0 for anything that is not a padded [n, d] view with 16-byte rows"""
    d, ld = t.shape[1], t.stride(0)
    return ld - d if (rows_vectored(t) and ld > d and t.stride(1) == 1) else 0


def padded_parent(t):
    """For a [n, d] view created by alloc_rows return the [n, ld] parent view (pad columns included)."""
    n, d = t.shape
    ld = t.stride(0) if n > 1 else row_pitch(d, elem_size=t.element_size())
    if ld == d:
        return t
    return torch.as_strided(t, (n, ld), (ld, 1), t.storage_offset())


MEM_MODES = {"default": _lib.SGL_MEM_DEFAULT, "contiguous": _lib.SGL_MEM_CONTIGUOUS, "vmm": _lib.SGL_MEM_VMM}


class _PlacedBlock:
    """device memory from sgl_mem_alloc, exported to torch through __cuda_array_interface__; freed with the last tensor"""

    def __init__(self, n_floats, mode, chunk_bytes, device):
        self.device = torch.device(device)
        self.n = int(n_floats)
        p = c_void_p()
        with torch.cuda.device(self.device):
            _lib.check_probe(_lib.probe_lib().sgl_mem_alloc(ctypes.byref(p), self.n * 4, MEM_MODES[mode], int(chunk_bytes)), f"sgl_mem_alloc({mode})")
        self.ptr = p.value
        self.__cuda_array_interface__ = {"shape": (self.n,), "typestr": "<f4", "data": (self.ptr, False), "version": 2}

    def __del__(self):
        p, self.ptr = getattr(self, "ptr", None), None
        if p:
            try:
                with torch.cuda.device(self.device):
                    _lib.probe_lib().sgl_mem_free(c_void_p(p))
            except Exception:
                pass


def placed_empty(shape, device, mode="contiguous", chunk_bytes=0):
    """float32 tensor of `shape` whose memory comes from sgl_mem_alloc with a stated physical placement (MEM_MODES).  For the
    multi-GB feature replicas the SpMM gathers from: a physically contiguous table is translated through far fewer TLB entries
    than whatever hipMalloc found free (profiles/r03_papers_tlb.md).  The block is released when the last view dies."""
    n = 1
    for s_ in shape:
        n *= int(s_)
    blk = _PlacedBlock(max(n, 1), mode, chunk_bytes, device)
    flat = torch.as_tensor(blk, device=blk.device)
    return flat[:n].view(*shape)


_STAGED_MIN_BYTES = 8 << 20     # below this a plain copy is as fast as the staging team


def upload_rows(x, device):
    """host ndarray / tensor [n, d] (any float dtype / order) -> padded device buffer view [n, d] float32"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    x = x.detach()
    n, d = x.shape
    out = alloc_rows(n, d, device)
    out.copy_(x.to(dtype=torch.float32), non_blocking=False)
    return out


def permute_rows(rowptr, col, val, perm):
    """the rows of a device CSR in the order `perm` (storage row k = input row perm[k]); column ids and every row's entries
    untouched (sgl_csr_permute_rows).  perm: int32 permutation on the device."""
    n = rowptr.numel() - 1
    perm = perm.to(torch.int32).contiguous()
    out_ptr = torch.empty(n + 1, dtype=torch.int64, device=rowptr.device)
    out_col = torch.empty_like(col)
    out_val = torch.empty_like(val)
    _call(rowptr.device, "sgl_csr_permute_rows", ptr(rowptr), ptr(col), ptr(val), n, ptr(perm), ptr(out_ptr), ptr(out_col), ptr(out_val))
    return out_ptr, out_col, out_val


def download_rows(t):
    """device [n, d] float32 (any row pitch) -> contiguous pageable CPU tensor, at link rate (sgl_download)"""
    src = t if t.is_contiguous() else t.contiguous()
    host = torch.empty(src.shape, dtype=torch.float32)
    if src.numel() * 4 < _STAGED_MIN_BYTES:
        host.copy_(src)
        return host
    _call(src.device, "sgl_download", host.data_ptr(), ptr(src), src.numel() * 4)
    return host


def _wrote(*tensors):
    """The library wrote into these caller-visible tensors through raw pointers: bump their torch version counters, as any in-place
    torch write would.  Whatever keys on (data_ptr, _version) -- autograd's saved-tensor checks, the content memo of
    hopcache.SharedHops, degree_powers' cache -- then sees the write."""
    for t in tensors:
        if torch.is_tensor(t):
            torch.autograd.graph.increment_version(t)


def _check_mat(t, name, bf16=False):
    """bf16=True: the entry point also has a bfloat16 form (bf16 hop storage)"""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and (t.dtype == torch.float32 or (bf16 and t.dtype == torch.bfloat16))):
        raise TypeError(f"{name} must be a 2-D float32{' or bfloat16' if bf16 else ''} CUDA tensor")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name} must be row-major (column stride 1)")
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        raise ValueError(f"{name}: row stride smaller than the row length")


def _same_hop_dtype(who, *tensors):
    """the one dtype of x / out (float32 or bfloat16): the bf16 entry points read and write bf16, nothing converts on the way"""
    dts = {t.dtype for t in tensors}
    if len(dts) != 1:
        raise TypeError(f"{who}: x and out must have the same dtype (float32 or bfloat16), got {sorted(str(d_) for d_ in dts)}")
    return dts.pop()


def _no_bf16(who, *tensors):
    if any(torch.is_tensor(t) and t.dtype == torch.bfloat16 for t in tensors):
        raise TypeError(f"{who} has no bfloat16 form (bf16 hop storage covers spmm, spmm_chain, spmm_acc, the row gathers and the "
                        "reduce / concat / NAFS aggregators)")


def widen_hops(feats):
    """bfloat16 hop matrices as float32 copies (exact), each in a padded buffer of its own; float32 ones are passed through.
    hop_reduce, hop_concat and nafs_aggregate read a list of bf16 hops in place and do not come here; what has no bf16 kernel does
    (hop_lincomb, nafs_prefix, the gradient-carrying wrappers, the learnable gates on whole matrices, lists that mix dtypes, the
    NAFS shapes the register-resident kernel does not take): the hops are widened hop by hop through torch and the fp32 kernels run
    -- a correctness fallback that costs 4 more bytes per element of every widened hop while the aggregate is computed."""
    out = []
    for f in feats:
        if torch.is_tensor(f) and f.is_cuda and f.dtype == torch.bfloat16 and f.dim() == 2:
            w = alloc_rows(f.shape[0], f.shape[1], f.device)
            w.copy_(f)
            f = w
        out.append(f)
    return out


def default_long_row_nnz(nnz):
    """where sgl_csr_create cuts long rows when it is not told (sgl::default_long_row_nnz, csrc/sgl_core.cpp: a function of the matrix's nnz only).  A row
    block of a sharded matrix has fewer non-zeros than the whole and would fall into another bracket: the distributed paths pass
    default_long_row_nnz(GLOBAL nnz) explicitly, so that the same rows are cut at the same places whatever the world size and the
    default-order hops of a sharded run stay bit-identical to the single-GPU run."""
    nnz = int(nnz)
    return 32 if nnz < (1 << 18) else 128 if nnz < (1 << 20) else 512 if nnz < (1 << 22) else 2048


class DeviceCSR:
    """A CSR matrix resident on one GPU plus its SpMM execution plan (sgl_csr_create).

    rowptr int64 [n_rows+1], col int32 [nnz], val float32 [nnz] -- CUDA tensors, kept alive here."""

    def __init__(self, rowptr, col, val, shape, strict=False, item_nnz=0, long_row_nnz=0, xcd_remap=True):
        _lib.require_gpu()
        for t, dt, nm in ((rowptr, torch.int64, "rowptr"), (col, torch.int32, "col"), (val, torch.float32, "val")):
            if not (t.is_cuda and t.dtype == dt and t.dim() == 1 and t.is_contiguous()):
                raise TypeError(f"{nm} must be a contiguous 1-D CUDA tensor of dtype {dt}")
        self.rowptr, self.col, self.val = rowptr, col, val
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz = int(col.numel())
        self.device = rowptr.device
        self.strict = bool(strict)
        flags = (_lib.SGL_CSR_STRICT_ORDER if strict else 0) | (0 if xcd_remap else _lib.SGL_CSR_NO_XCD_REMAP)
        h = c_void_p()
        _call(self.device, "sgl_csr_create", ctypes.byref(h), self.shape[0], self.shape[1], self.nnz, ptr(rowptr), ptr(col), ptr(val),
              flags, int(item_nnz), int(long_row_nnz))
        self._h = h

    @classmethod
    def from_scipy(cls, adj, device="cuda", **kw):
        """scipy CSR (any float dtype; values rounded to float32 here, where the reference rounds them,
        operators/utils.py:32) -> device."""
        import scipy.sparse as sp
        if not sp.isspmatrix_csr(adj):
            raise TypeError("expected a scipy.sparse.csr_matrix")
        rowptr = torch.from_numpy(adj.indptr.astype(np.int64)).to(device)
        col = torch.from_numpy(adj.indices.astype(np.int32)).to(device)
        val = torch.from_numpy(adj.data.astype(np.float32)).to(device)
        return cls(rowptr, col, val, adj.shape, **kw)

    def set_values(self, val):
        """same sparsity structure, new values (another normalisation of the same graph): the execution plan is kept"""
        if not (val.is_cuda and val.dtype == torch.float32 and val.dim() == 1 and val.is_contiguous() and val.numel() == self.nnz):
            raise TypeError("val must be a contiguous float32 CUDA tensor with one entry per non-zero")
        _call(None, "sgl_csr_set_values", self._h, ptr(val))
        self.val = val
        return self

    rowmap = None

    def set_rowmap(self, rowmap):
        """the handle's rows are stored in processing order: storage row i is output row rowmap[i] (int32 permutation on the
        device, kept alive here; None removes it).  sgl_csr_set_rowmap."""
        if rowmap is not None and not (rowmap.is_cuda and rowmap.dtype == torch.int32 and rowmap.dim() == 1
                                       and rowmap.is_contiguous() and rowmap.numel() == self.shape[0]):
            raise TypeError("rowmap must be a contiguous int32 CUDA tensor with one entry per row")
        _call(self.device, "sgl_csr_set_rowmap", self._h, _opt_ptr(rowmap))
        self.rowmap = rowmap
        return self

    def info(self):
        a = (c_int64 * 8)()
        _call(None, "sgl_csr_info", self._h, a)
        keys = ("n_rows", "n_cols", "nnz", "n_items", "n_pieces", "n_long_rows", "flags", "workspace_bytes")
        return dict(zip(keys, list(a)))

    def spmm(self, x, out=None, accumulate=False):
        """out = A @ x (+ out when accumulate).  x: [n_cols, d] float32 CUDA row-major; returns [n_rows, d].
        A bfloat16 x (and out) runs sgl_spmm_bf16: bf16 in, fp32 accumulation, one rounding to bf16 out; no accumulate form."""
        _check_mat(x, "x", bf16=True)
        if x.shape[0] != self.shape[1]:
            raise ValueError("Dimension mismatch detected for the adjacency and the feature matrix!")
        d = x.shape[1]
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs an `out` tensor")
            out = alloc_rows(self.shape[0], d, x.device, zero_pad=True, dtype=x.dtype)
        else:
            _check_mat(out, "out", bf16=True)
            if out.shape != (self.shape[0], d):
                raise ValueError("out has the wrong shape")
        if _same_hop_dtype("spmm", x, out) == torch.bfloat16:
            if accumulate:
                raise ValueError("spmm: bfloat16 hops have no accumulate form")
            _call(self.device, "sgl_spmm_bf16", self._h, ptr(x), _ld(x), ptr(out), _ld(out), d)
        else:
            _call(self.device, "sgl_spmm_f32", self._h, ptr(x), _ld(x), ptr(out), _ld(out), d, int(bool(accumulate)))
        _wrote(out)
        return out

    ACC_MODES = {kind: acc for kind, (_, acc) in HOP_KINDS.items() if acc is not None}

    def spmm_acc(self, x, out, acc, w=1.0, weighted=False, divisor=1.0, mode=None):
        """out = A @ x and, in the same kernel, acc <- acc + out (weighted: acc + w * out), then acc / divisor if
        divisor != 1, or acc <- max / min(acc, out) (sgl_spmm_acc_f32): the running hop aggregate of Sum / Mean /
        SimpleWeighted / Max / Min"""
        mode = self.ACC_MODES[mode] if mode is not None else int(bool(weighted))
        _check_mat(x, "x", bf16=True)
        _check_mat(out, "out", bf16=True)
        _check_mat(acc, "acc")
        if x.shape[0] != self.shape[1] or out.shape != (self.shape[0], x.shape[1]) or acc.shape != out.shape:
            raise ValueError("Dimension mismatch detected for the adjacency and the feature matrix!")
        bf16 = _same_hop_dtype("spmm_acc", x, out) == torch.bfloat16        # bf16 hops: acc stays float32 and takes the ROUNDED out
        _call(self.device, "sgl_spmm_acc_bf16" if bf16 else "sgl_spmm_acc_f32", self._h, ptr(x), _ld(x), ptr(out), _ld(out), x.shape[1],
              ptr(acc), _ld(acc), float(w), mode, float(divisor))
        _wrote(out, acc)
        return out

    def spmm_multi(self, x, out_ptrs, ld, row_mask=None):
        """A @ x stored into several [n_rows, d] matrices given as RAW device addresses (the first is normally local,
        the others peer-GPU replicas mapped through IPC) with leading dimension `ld`.  row_mask: optional uint8 CUDA
        tensor [n_rows]; bit q set = destination q+1 gets that row."""
        _no_bf16("spmm_multi", x)
        _check_mat(x, "x")
        if x.shape[0] != self.shape[1]:
            raise ValueError("Dimension mismatch detected for the adjacency and the feature matrix!")
        n_out = len(out_ptrs)
        if not 1 <= n_out <= 8:
            raise ValueError("between 1 and 8 output replicas are supported")
        arr = (c_void_p * n_out)(*[int(p) for p in out_ptrs])
        if row_mask is not None and not (row_mask.is_cuda and row_mask.dtype == torch.uint8 and row_mask.is_contiguous()
                                         and row_mask.numel() == self.shape[0]):
            raise ValueError("row_mask must be a contiguous uint8 CUDA tensor with one entry per row")
        _call(self.device, "sgl_spmm_multi_f32", self._h, ptr(x), _ld(x), n_out, arr, int(ld), x.shape[1], _opt_ptr(row_mask))

    def spmm_chain(self, x, n_hops, outs=None):
        """[A x, A^2 x, ..., A^k x] with ONE library call (the hop loop runs in C).  x: [n, d] row-major CUDA; the
        results are row-padded buffers of the same width and dtype as x (or the caller's `outs`).  bfloat16 x: sgl_spmm_chain_bf16,
        every hop rounded once to bf16 and read back as such by the next."""
        _check_mat(x, "x", bf16=True)
        if x.shape[0] != self.shape[1] or self.shape[0] != self.shape[1]:
            raise ValueError("Dimension mismatch detected for the adjacency and the feature matrix!")
        d = x.shape[1]
        if outs is None:
            outs = [alloc_rows(self.shape[0], d, x.device, zero_pad=True, dtype=x.dtype) for _ in range(n_hops)]
        else:
            if len(outs) != n_hops:
                raise ValueError("need one output matrix per hop")
            for o in outs:
                _check_mat(o, "outs[*]", bf16=True)
                if o.shape != (self.shape[0], d):
                    raise ValueError("an output matrix has the wrong shape")
        if n_hops:
            bf16 = _same_hop_dtype("spmm_chain", x, *outs) == torch.bfloat16
            ptrs, lds = _lib.hop_arrays(outs, one_row_pitch=False)
            _call(self.device, "sgl_spmm_chain_bf16" if bf16 else "sgl_spmm_chain_f32", self._h, n_hops, ptr(x), _ld(x), ptrs, lds, d)
            _wrote(*outs)
        return outs

    def capture_chain(self, x, outs):
        """hipGraph of `spmm_chain(x, len(outs), outs)`: returns a ChainGraph whose replay() re-runs the k hops on the
        current stream with one launch (x and outs are baked in: refill x in place between replays)."""
        _no_bf16("capture_chain", x, *outs)
        _check_mat(x, "x")
        for o in outs:
            _check_mat(o, "outs[*]")
            if o.shape != (self.shape[0], x.shape[1]):
                raise ValueError("an output matrix has the wrong shape")
        ptrs, lds = _lib.hop_arrays(outs, one_row_pitch=False)
        g = c_void_p()
        torch.cuda.synchronize(self.device)
        _call(self.device, "sgl_chain_graph_create", ctypes.byref(g), self._h, len(outs), ptr(x), _ld(x), ptrs, lds, x.shape[1])
        return ChainGraph(g, self, x, list(outs))

    def spmm_axpb_clamp(self, x, alpha, res=None, lo=float("-inf"), hi=float("inf"), out=None):
        """out = clamp(alpha * (A @ x) + res, lo, hi) in one kernel (the label-propagation step)"""
        _no_bf16("spmm_axpb_clamp", x, res, out)
        _check_mat(x, "x")
        if x.shape[0] != self.shape[1]:
            raise ValueError("Dimension mismatch detected for the adjacency and the feature matrix!")
        d = x.shape[1]
        if out is None:
            out = alloc_rows(self.shape[0], d, x.device, zero_pad=True)
        else:
            _check_mat(out, "out")
        if res is not None:
            _check_mat(res, "res")
            if res.shape != (self.shape[0], d):
                raise ValueError("res has the wrong shape")
        _call(self.device, "sgl_spmm_axpb_clamp_f32", self._h, ptr(x), _ld(x), ptr(out), _ld(out), d, float(alpha), _opt_ptr(res),
              _ld(res) if res is not None else 0, float(lo), float(hi))
        _wrote(out)
        return out

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _call(None, "sgl_csr_destroy", h, raw=True)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class ChainGraph:
    """a captured k-hop propagation (DeviceCSR.capture_chain); keeps the matrix and the buffers alive"""

    def __init__(self, handle, csr, x, outs):
        self._g, self.csr, self.x, self.outs = handle, csr, x, outs

    def replay(self):
        _call(self.csr.device, "sgl_chain_graph_launch", self._g)
        _wrote(*self.outs)
        return self.outs

    def close(self):
        g, self._g = getattr(self, "_g", None), None
        if g:
            _call(None, "sgl_chain_graph_destroy", g, raw=True)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


_POW_CACHE = []          # at most one entry: (deg tensor, its version counter, r, host_pow, left, right)
_POW_THREADS = max(1, min(64, (os.cpu_count() or 2) // 2))
pow_stats = {"cache_hits": 0, "host_unique": 0, "host_full": 0, "device": 0}


def _host_powers(d, r):
    """numpy's deg^(r-1), deg^(-r) with inf -> 0 (utils.py:79-84) on a 1-D float64 array, written into two new arrays; long
    vectors are cut into chunks evaluated by a team of threads (the ufunc loop releases the GIL; the values do not depend on the cut)"""
    left, right = np.empty_like(d), np.empty_like(d)

    def run(a, b):
        with np.errstate(divide="ignore", invalid="ignore"):
            np.power(d[a:b], r - 1, out=left[a:b])
            left[a:b][np.isinf(left[a:b])] = 0.
            np.power(d[a:b], -r, out=right[a:b])
            right[a:b][np.isinf(right[a:b])] = 0.
    n = d.shape[0]
    chunk = 1 << 20
    if n <= 2 * chunk or _POW_THREADS == 1:
        run(0, n)
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(_POW_THREADS) as ex:
            list(ex.map(lambda a: run(a, min(a + chunk, n)), range(0, n, chunk)))
    return left, right


def _few_distinct(deg, sample=4096):
    """cheap guess BEFORE sorting the whole vector: do evenly spaced samples repeat each other?  (unit-weight graphs: a few
    hundred distinct degrees among millions of nodes; real-valued weights: every degree its own)"""
    n = deg.numel()
    if n <= 4 * sample:
        return True
    s = deg[:: n // sample][:sample]
    return torch.unique(s).numel() * 2 <= s.numel()


def degree_powers(deg, r, host_pow=True):
    """deg^(r-1), deg^(-r) with inf -> 0 (operators/utils.py:79-84) as two fp64 tensors on deg's device.

    host_pow=True: evaluated on the HOST by numpy exactly as the reference does: the same routine, hence bit-identical
    degree factors and a bit-identical A_hat.  Only the DISTINCT degree values travel when there are few of them (a unit-weight
    graph has far fewer distinct degrees than nodes: 2.4 M nodes -> a few thousand values; a strided sample decides, so a
    vector of all-distinct real-valued degrees is never sorted); otherwise the vector goes through pinned buffers and a team of
    host threads.  host_pow=False: the device's pow() (sgl_norm_degree_powers), within 1 ulp(fp64) of the host's -- A_hat then
    differs from the reference's in the last fp32 bit of a handful of entries (tests: <= 1 ulp), far inside the 1e-5 contract.
    host_pow="auto": the host route when the degrees have few distinct values (it then costs microseconds), the device otherwise.
    The last result is cached per (degree vector, r, route): an alpha sweep, or re-normalising the same graph, pays once."""
    r = float(r)
    for ent in _POW_CACHE:
        if ent[0] is deg and ent[1] == deg._version and ent[2] == r and ent[3] == host_pow:
            pow_stats["cache_hits"] += 1
            return ent[4], ent[5]
    asked = host_pow
    few = None
    if host_pow == "auto":
        # host route (bit-identical to the reference) whenever it is cheap -- few distinct degrees: every unit-weight graph --
        # the device's pow() when every node has its own real-valued degree
        few = (not deg.is_cuda) or deg.numel() <= 4096 or _few_distinct(deg)
        host_pow = few
    if deg.is_cuda and not host_pow:
        left, right = torch.empty_like(deg), torch.empty_like(deg)
        _call(deg.device, "sgl_norm_degree_powers", deg.numel(), ptr(deg), r, ptr(left), ptr(right))
        pow_stats["device"] += 1
    elif deg.is_cuda and deg.numel() > 4096 and (few if few is not None else _few_distinct(deg)):
        uniq, inv = torch.unique(deg, return_inverse=True)
        lu, ru = _host_powers(uniq.cpu().numpy(), r)
        left, right = torch.from_numpy(lu).to(deg.device)[inv], torch.from_numpy(ru).to(deg.device)[inv]
        pow_stats["host_unique"] += 1
    elif deg.is_cuda:
        from . import hostpool
        n = deg.numel()
        bufs = [hostpool.take((n,), torch.float64) if n >= (1 << 20) else None for _ in range(3)]
        h = bufs[0] if bufs[0] is not None else torch.empty(n, dtype=torch.float64)
        h.copy_(deg)
        hl, hr = _host_powers(h.numpy(), r)
        outs = []
        for src, buf in ((hl, bufs[1]), (hr, bufs[2])):
            t = torch.from_numpy(src)
            if buf is not None:
                buf.copy_(t)
                t = buf
            outs.append(t.to(deg.device, non_blocking=buf is not None))
        torch.cuda.current_stream(deg.device).synchronize()      # the pinned buffers go back to the pool
        left, right = outs
        pow_stats["host_full"] += 1
    else:
        hl, hr = _host_powers(deg.detach().numpy().astype(np.float64, copy=False), r)
        left, right = torch.from_numpy(hl), torch.from_numpy(hr)
    _POW_CACHE[:] = [(deg, deg._version, r, asked, left, right)]
    return left, right


def clear_power_cache():
    _POW_CACHE.clear()


def _all_positive(val, deg=None):
    """one flag per preparation: is every stored weight of A (and every degree handed in) > 0?  Then A + I holds no stored zero and
    no degree is 0, so no entry of A_hat can be exactly 0 and the kernels' union pattern of A and I IS the reference's.  Anything
    else -- a stored 0, a negative or NaN weight, a_ii = -1, a degree <= 0 -- may leave exact zeros behind, which scipy never
    stores (_drop_exact_zeros).  Two reductions and one read-back per preparation, none per (r, alpha)."""
    flags = [t.min() > 0 for t in (val, deg) if t is not None and t.numel()]
    return bool(torch.stack(flags).all().item()) if flags else True


def _drop_exact_zeros(rowptr, col, val32, val64):
    """(rowptr, col, val32, val64) without the entries whose fp64 value is exactly 0 (NaN is kept): what scipy leaves of them -- it
    stores no exact zero after A + I, after either diagonal product, or after the PPR sum (operators/utils.py:77-87,
    ppr_graph_op.py:20).  Only ever entered for a preparation that _all_positive() did not clear (or alpha = 1); the inputs are
    left as they are, so a cached Laplacian and the diagonal positions keep describing the uncompacted block."""
    keep = val64 != 0
    if bool(keep.all().item()):
        return rowptr, col, val32, val64
    before = torch.zeros(keep.numel() + 1, dtype=torch.int64, device=keep.device)
    before[1:] = torch.cumsum(keep, 0)
    return before[rowptr], col[keep], val32[keep], val64[keep]


def _reference_pattern(prune, return_fp64, rowptr, col, values):
    """the tail of every normalize(): `values` = (val32, val64) over (rowptr, col) when `prune` (the preparation may hold a zero,
    or alpha = 1: (1 - alpha) A_hat is all zeros and the reference keeps alpha I alone), else what the caller asked for"""
    if prune:
        rowptr, col, v32, v64 = _drop_exact_zeros(rowptr, col, *values)
        values = (v32, v64) if return_fp64 else (v32,)
    return (rowptr, col) + values


class PreparedAdjacency:
    """A + I of a whole matrix on the device (CSR, fp64 values), its row sums = degrees, and whether A is symmetric --
    everything about a graph that does not depend on r / alpha (sgl_norm_build_symcheck).  One preparation serves every
    normalisation of the same graph: the r-sweep of the NAFS task, the alpha-sweep of a PaSca search."""

    def __init__(self, rowptr, col, val, n):
        _lib.require_gpu()
        dev = rowptr.device
        nnz = int(col.numel())
        self.n, self.src = int(n), (rowptr, col, val)
        nnz_out = c_int64(0)
        with torch.cuda.device(dev):
            _call(dev, "sgl_norm_block_prepare", n, 0, nnz, ptr(rowptr), ptr(col), ctypes.byref(nnz_out))
            m = nnz_out.value
            self.rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
            self.col = torch.empty(m, dtype=torch.int32, device=dev)
            self.t64 = torch.empty(m, dtype=torch.float64, device=dev)
            self.deg = torch.empty(n, dtype=torch.float64, device=dev)
            fp = torch.zeros(1, dtype=torch.int64, device=dev)
            _call(dev, "sgl_norm_build_symcheck", n, nnz, ptr(rowptr), ptr(col), ptr(val), m, ptr(self.rowptr), ptr(self.col),
                  ptr(self.t64), ptr(self.deg), ptr(fp))
            # one read-back for both answers: is A symmetric, and can an entry of A_hat be exactly 0 (see _all_positive)
            ok = val.min() > 0 if nnz else torch.ones((), dtype=torch.bool, device=dev)
            asym, ok = torch.stack([fp[0] != 0, ok]).tolist()
            self.symmetric, self.may_hold_zero = not asym, not ok
        self.nnz_out = m
        self.device = dev
        if self.symmetric:
            self.src = None            # the raw matrix is only needed again for the one-off transposition of a directed graph

    def nbytes(self):
        """device bytes this object keeps alive beyond the caller's own matrix (A + I in fp64, degrees, cached Laplacian, ...)"""
        seen, total = set(), 0
        objs = [self] + ([self.__dict__["_tblock"]] if self.__dict__.get("_tblock") is not None else [])
        for o in objs:
            for name, v in o.__dict__.items():
                if name == "src":
                    continue
                if isinstance(v, tuple) and len(v) == 2 and torch.is_tensor(v[1]):
                    v = v[1]                                         # _hat64 = (key, tensor)
                if torch.is_tensor(v) and v.is_cuda and v.data_ptr() not in seen:
                    seen.add(v.data_ptr())
                    total += v.numel() * v.element_size()
        return total

    def drop_values(self):
        """release the cached fp64 Laplacian of the last PPR request (8 bytes per non-zero)"""
        self.__dict__["_hat64"] = None
        tb = self.__dict__.get("_tblock")
        if tb is not None:
            tb.drop_values()

    def normalize(self, r, alpha=None, return_fp64=False, host_pow=True):
        """A_hat for this (r, alpha).  Symmetric A: one scaling pass over A + I, A_hat[j,i] = (A'[j,i] L[j]) R[i] -- no
        transposition; otherwise the transpose is built once (one stable sort) and every (r, alpha) is the same single pass over it.
        Both are bit-identical to the reference's scipy result (host_pow=True; see degree_powers).  PPR requests keep the fp64
        Laplacian of their r: the next alpha of a sweep is one stream over it (sgl_norm_block_mix), bit-identical to the one-pass form."""
        dev = self.device
        with torch.cuda.device(dev):
            if self.symmetric:
                prune = self.may_hold_zero or alpha == 1.0
                vals = _scaled_values(self, self.n, 0, self.rowptr, self.col, self.t64, self.deg, r, alpha, return_fp64 or prune,
                                      host_pow)
                return _reference_pattern(prune, return_fp64, self.rowptr, self.col, vals)
            # directed / value-asymmetric A: A_hat[j, i] = (T'[j, i] L[j]) R[i] with T = A^T.  The transposition (one stable sort:
            # sgl_coo_to_csr with rows and columns swapped) does not depend on (r, alpha) either: done ONCE, after which every
            # (r, alpha) is the same single pass as in the symmetric case -- 2 ms instead of the 21 ms of the general pipeline
            # (sgl_norm_execute_lr re-sorts per call) at the products shape.  The degrees stay the sequential row sums of A + I
            # computed above (scipy's order), so the result is bit-identical to the general pipeline and to the reference.
            tb = self.__dict__.get("_tblock")
            if tb is None:
                from .io import coo_to_csr_device
                rowptr, col, val = self.src
                rows = torch.repeat_interleave(torch.arange(self.n, dtype=torch.int64, device=dev), rowptr[1:] - rowptr[:-1])
                t = coo_to_csr_device(col.to(torch.int64), rows, val, self.n, device=dev)
                tb = self._tblock = PreparedBlock(t.rowptr, t.col, t.val, 0, self.n, symmetric=False, deg=self.deg)
                self.rowptr = self.col = self.t64 = self.src = None   # neither A + I nor the raw matrix is needed any more
            return tb.normalize(r, alpha, return_fp64=return_fp64, host_pow=host_pow)


def _scaled_values(owner, n_loc, row0, rowptr, col, t64, deg, r, alpha, return_fp64, host_pow, keep_hat64=None):
    """the (r, alpha)-dependent pass over a prepared T' = T + I (rows [row0, row0 + n_loc), global column ids; `deg` = the global
    degree vector): returns (val32,) or (val32, val64).  `owner` carries the one-entry cache of the fp64 Laplacian values
    (`_hat64` = ((r, host_pow), tensor)): kept when a PPR matrix is asked for (or keep_hat64=True), so that the other alphas of a
    sweep at the same r skip the degree factors and the R gather altogether."""
    dev = rowptr.device
    m = int(col.numel())
    key = (float(r), host_pow)
    keep = (alpha is not None) if keep_hat64 is None else bool(keep_hat64)
    cached = getattr(owner, "_hat64", None)
    hat64 = cached[1] if (cached is not None and cached[0] == key) else None
    o_val = torch.empty(m, dtype=torch.float32, device=dev)
    o_v64 = torch.empty(m, dtype=torch.float64, device=dev) if return_fp64 else None
    if hat64 is None:
        left, right = degree_powers(deg, r, host_pow)
        left_loc = left if (row0 == 0 and n_loc == left.numel()) else left[row0:row0 + n_loc].contiguous()
        if alpha is None or not keep:
            if keep:                                 # Laplacian asked for, values to be kept: the fp64 output IS the cache entry
                o_v64 = o_v64 if o_v64 is not None else torch.empty(m, dtype=torch.float64, device=dev)
            _call(dev, "sgl_norm_block_scale", n_loc, row0, ptr(rowptr), ptr(col), ptr(t64), ptr(left_loc), ptr(right),
                  int(alpha is not None), float(alpha if alpha is not None else 0.0), ptr(o_val), _opt_ptr(o_v64))
            if keep:
                owner._hat64 = (key, o_v64)
                if return_fp64:
                    o_v64 = o_v64.clone()            # the caller may edit what it gets; the cache entry stays private
            return (o_val, o_v64) if return_fp64 else (o_val,)
        # PPR with the cache empty: the Laplacian in fp64 first (o_val is scratch for its fp32 rounding), then the mix below
        hat64 = torch.empty(m, dtype=torch.float64, device=dev)
        _call(dev, "sgl_norm_block_scale", n_loc, row0, ptr(rowptr), ptr(col), ptr(t64), ptr(left_loc), ptr(right), 0, 0.0, ptr(o_val),
              ptr(hat64))
        owner._hat64 = (key, hat64)
    if alpha is None:
        # Laplacian again at a cached r: alpha = 0 would multiply by 1.0 and add 0.0 to the diagonal -- exact, but a plain rounding
        # pass says what it does
        o_val.copy_(hat64)
        return (o_val, hat64.clone()) if return_fp64 else (o_val,)
    diag = getattr(owner, "_diag", None)
    if diag is None:                                  # where each row's diagonal entry sits: once per prepared block
        diag = torch.empty(n_loc, dtype=torch.int64, device=dev)
        _call(dev, "sgl_norm_block_diag_positions", n_loc, row0, ptr(rowptr), ptr(col), ptr(diag))
        owner._diag = diag
    _call(dev, "sgl_norm_block_mix_at", m, n_loc, ptr(hat64), ptr(diag), float(alpha), ptr(o_val), ptr(o_v64) if return_fp64 else None)
    return (o_val, o_v64) if return_fp64 else (o_val,)


def normalize_adj(rowptr, col, val, n, r, alpha=None, return_fp64=False, host_pow=True, prepared=None):
    """Device adj_to_symmetric_norm (+ optional PPR mix): canonical CSR of A on device -> CSR of A_hat.
    rowptr int64 [n+1], col int32, val float32 (CUDA).  Returns (rowptr, col, val[, val64]).
    host_pow (default): the two degree powers are evaluated by the host's numpy like the reference's, everything per
    non-zero stays on the GPU; the rounded A_hat is then bit-identical to scipy's.  `prepared`: a PreparedAdjacency of the
    same matrix (re-used across r / alpha); host_pow=False is the all-device pipeline with the GPU's pow().
    The pattern is the reference's on every route: entries that come out exactly 0 (stored zeros of A, a_ii = -1, a degree of
    0) are not returned, as scipy does not store them (_drop_exact_zeros; graphs of positive weights never get there)."""
    _lib.require_gpu()
    if host_pow or prepared is not None:
        prep = prepared if prepared is not None else PreparedAdjacency(rowptr, col, val, n)
        return prep.normalize(r, alpha, return_fp64=return_fp64, host_pow=host_pow)
    nnz = int(col.numel())
    dev = rowptr.device
    nnz_out = c_int64(0)
    with torch.cuda.device(dev):
        _call(dev, "sgl_norm_prepare", n, nnz, ptr(rowptr), ptr(col), ctypes.byref(nnz_out))
        m = nnz_out.value
        o_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        o_col = torch.empty(m, dtype=torch.int32, device=dev)
        o_val = torch.empty(m, dtype=torch.float32, device=dev)
        prune = not _all_positive(val) or alpha == 1.0
        o_v64 = torch.empty(m, dtype=torch.float64, device=dev) if (return_fp64 or prune) else None
        _call(dev, "sgl_norm_execute", n, nnz, ptr(rowptr), ptr(col), ptr(val), float(r), int(alpha is not None),
              float(alpha if alpha is not None else 0.0), m, ptr(o_ptr), ptr(o_col), ptr(o_val), _opt_ptr(o_v64))
        # the C entry point keeps the union pattern of A and I; the reference's pattern is this layer's business
        return _reference_pattern(prune, return_fp64, o_ptr, o_col, (o_val, o_v64) if o_v64 is not None else (o_val,))


class PreparedBlock:
    """Everything about ONE RANK'S row block that does not depend on (r, alpha): T' = T + I for rows [row0, row0 + n_local) of
    T = A^T (symmetric=True: of A itself) as CSR with fp64 values (sgl_norm_block_build), and the GLOBAL degree vector of A + I
    (`deg`, fp64 [n_cols]).  The only communication is that vector: the blocks' row sums when A is symmetric, an all-reduce of
    the column sums otherwise; a caller that already holds it passes `deg=` and nothing is communicated.  One preparation then
    serves every normalize(r, alpha) of the block: the degree factors are cached per r (degree_powers), a PPR sweep keeps the
    fp64 Laplacian of its r, so (r, alpha) costs one pass over the block -- what a PaSca sweep over graph operators pays per
    candidate (sgl/search/search_config.py:14-15)."""

    def __init__(self, rowptr, col, val, row0, n_cols, symmetric=True, group=None, deg=None):
        import torch.distributed as dist
        _lib.require_gpu()
        dev = rowptr.device
        n_loc = int(rowptr.numel()) - 1
        nnz = int(col.numel())
        nnz_out = c_int64(0)
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
        self.n_local, self.row0, self.n_cols, self.symmetric = n_loc, int(row0), int(n_cols), bool(symmetric)
        with torch.cuda.device(dev):
            _call(dev, "sgl_norm_block_prepare", n_loc, row0, nnz, ptr(rowptr), ptr(col), ctypes.byref(nnz_out))
            m = nnz_out.value
            self.rowptr = torch.empty(n_loc + 1, dtype=torch.int64, device=dev)
            self.col = torch.empty(m, dtype=torch.int32, device=dev)
            self.t64 = torch.empty(m, dtype=torch.float64, device=dev)
            rowsum = torch.empty(n_loc, dtype=torch.float64, device=dev)
            _call(dev, "sgl_norm_block_build", n_loc, row0, nnz, ptr(rowptr), ptr(col), ptr(val), m, ptr(self.rowptr), ptr(self.col),
                  ptr(self.t64), ptr(rowsum))
            if deg is not None:
                if deg.numel() != n_cols:
                    raise ValueError("deg must hold one entry per column")
                deg = deg.to(dev)
            elif symmetric:
                if multi:
                    deg = torch.zeros(n_cols, dtype=torch.float64, device=dev)
                    deg[row0:row0 + n_loc] = rowsum
                    dist.all_reduce(deg, group=group)      # blocks are disjoint: the sum IS the concatenation (exact)
                else:
                    if n_loc != n_cols or row0 != 0:
                        raise ValueError("a single process must hold the whole matrix")
                    deg = rowsum
            else:
                deg = torch.zeros(n_cols, dtype=torch.float64, device=dev)
                _call(dev, "sgl_norm_block_colsum", n_cols, m, ptr(self.col), ptr(self.t64), ptr(deg))
                if multi:
                    dist.all_reduce(deg, group=group)
            self.may_hold_zero = not _all_positive(val, deg)
        self.deg = deg
        self.nnz_out = m
        self._hat64 = None

    def normalize(self, r, alpha=None, return_fp64=False, host_pow=True, keep_hat64=None):
        """(rowptr, col, val[, val64]) of this block of A_hat (local row pointers, global column ids)"""
        with torch.cuda.device(self.rowptr.device):
            prune = self.may_hold_zero or alpha == 1.0
            vals = _scaled_values(self, self.n_local, self.row0, self.rowptr, self.col, self.t64, self.deg, r, alpha,
                                  return_fp64 or prune, host_pow, keep_hat64)
            return _reference_pattern(prune, return_fp64, self.rowptr, self.col, vals)

    def drop_values(self):
        """release the cached fp64 Laplacian (8 bytes per non-zero)"""
        self._hat64 = None


def normalize_block(rowptr, col, val, row0, n_cols, r, alpha=None, symmetric=True, group=None, return_fp64=False, deg=None,
                    host_pow=True, prepared=None):
    """Rows [row0, row0 + n_local) of A_hat from the same rows of T = A^T (symmetric=True: of A itself), each rank of a
    row-sharded job on its own block (sgl_norm_block_*).  The only communication is the degree vector: an all-gather of
    the blocks' row sums when A is symmetric, an all-reduce of the column sums otherwise.  Without an initialised
    process group (or world size 1) the block must be the whole matrix.  Returns (rowptr, col, val[, val64]) of the block
    (local row pointers, global column ids).  `deg` (fp64 [n_cols], any device): the global degree vector of A + I if
    the caller already has it -- then nothing is communicated at all.  `prepared`: a PreparedBlock of the same block (the
    (r, alpha)-independent part, re-used across a sweep); host_pow: see degree_powers (True = bit-identical to the reference)."""
    prep = prepared if prepared is not None else PreparedBlock(rowptr, col, val, row0, n_cols, symmetric=symmetric, group=group, deg=deg)
    return prep.normalize(r, alpha, return_fp64=return_fp64, host_pow=host_pow, keep_hat64=None if prepared is not None else False)


# ------------------------------------------------------------------------------------------------
# aggregators
# ------------------------------------------------------------------------------------------------
def _check_hops(feats, bf16=False):
    """bf16=True: a list that _all_bf16() accepted, for an entry point that reads bfloat16 hops in place"""
    if len(feats) < 1 or len(feats) > _lib.SGL_MAX_HOPS:
        raise ValueError(f"between 1 and {_lib.SGL_MAX_HOPS} hop matrices are supported")
    for i, f in enumerate(feats):
        _check_mat(f, f"feat_list[{i}]", bf16=bf16)
        if f.shape != feats[0].shape or f.device != feats[0].device:
            raise ValueError("all hop matrices must have the same shape and device")


def _widened(feats, out):
    """For d % 4 != 0: when every hop matrix and the (freshly allocated) output are row-padded to a multiple of
    4 floats, run element-wise kernels over the padded width so they use 16-byte lanes.  Inputs' pad columns are
    only read, the output's pad columns belong to us."""
    n, d = out.shape
    strides = {t.stride(0) for t in list(feats) + [out]} if n > 1 else set()
    if len(strides) == 1 and pitch_vectored(out) and out.stride(0) > d:
        dp = out.stride(0)            # every buffer has the same pitch: stream whole rows, pad included (contiguous)
    else:
        dp = round_up(d, 4)
    if d == dp or n <= 1:
        return feats, out, d
    if not all(rows_vectored(f, width=dp) for f in list(feats) + [out]):
        return feats, out, d
    wide = [torch.as_strided(f, (n, dp), (f.stride(0), 1), f.storage_offset()) for f in feats]
    return wide, torch.as_strided(out, (n, dp), (out.stride(0), 1), out.storage_offset()), dp


def _all_bf16(feats):
    """every member a bfloat16 CUDA matrix: the list goes to a kernel that reads bf16 hops in place, nothing is copied"""
    return len(feats) > 0 and all(torch.is_tensor(f) and f.is_cuda and f.dim() == 2 and f.dtype == torch.bfloat16 for f in feats)


def _alloc_out(n, d, device, dtype=torch.float32):
    """(alloc_rows output, its own_pad) for a kernel that writes the declared pad columns itself, as zeros; where there is padding
    the kernel is not told about (a single row), it is zeroed here"""
    out = alloc_rows(n, d, device, zero_pad=False, dtype=dtype)
    pad = own_pad(out)
    if pad == 0:
        parent = padded_parent(out)
        if parent.shape[1] != d:
            parent[:, d:].zero_()
    return out, pad


def _grad_rows(gout, n, d):
    """the incoming gradient of a [n, d] result as a detached float32 row-major matrix (copied only when it is not one)"""
    g = gout.detach().to(torch.float32)
    if g.stride(1) != 1 or (n > 1 and g.stride(0) < d):
        g = g.contiguous()
    return g


def hop_reduce(op, feats, weights=None):
    """sum / mean / max / min / 1-D weighted sum over the hop list -> new [n, d] float32 tensor.  A list of bfloat16 hops is read in
    place (sgl_hop_reduce_bf16_f32: every element widened exactly, the float32 kernel's operations in its order -- the same bits
    as over widened copies, without the copies); a list that mixes dtypes widens its bfloat16 members first (widen_hops) and runs
    sgl_hop_reduce_f32."""
    direct = _all_bf16(feats)
    if not direct:
        feats = widen_hops(feats)
    _check_hops(feats, bf16=direct)
    n, d = feats[0].shape
    device = feats[0].device
    w = None
    if op == _lib.SGL_REDUCE_WSUM:
        w = weights.detach().to(device=device, dtype=torch.float32).contiguous()
        if w.numel() != len(feats):
            raise ValueError("The feature list and the weight list have different lengths!")
    if direct:                     # the kernel writes the pad columns it is told about, as zeros
        result, pad = _alloc_out(n, d, device)
        name, out, pad = "sgl_hop_reduce_bf16_f32", result, (pad,)
    else:                          # element-wise over the padded width where every matrix has one (pad columns: zeros in, zeros out)
        result = alloc_rows(n, d, device)
        feats, out, d = _widened(feats, result)
        name, pad = "sgl_hop_reduce_f32", ()
    ptrs, lds = _lib.hop_arrays(feats)
    _call(device, name, op, len(feats), ptrs, lds, _opt_ptr(w), ptr(out), _ld(out), *pad, n, d)
    return result


def hop_concat(feats, out_dtype=None):
    """the hops side by side -> [n, H d] float32 (sgl_hop_concat_padded_f32).  A list of bfloat16 hops is read in place
    (sgl_hop_concat_bf16_f32: an exact widening), and with out_dtype=torch.bfloat16 stays bfloat16 (sgl_hop_concat_bf16: a copy of bit
    patterns into an alloc_rows(..., dtype=torch.bfloat16) matrix); a list that mixes dtypes widens its bfloat16 members first
    (widen_hops)."""
    if out_dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError(f"hop_concat: out_dtype is float32 or bfloat16, not {out_dtype}")
    direct = _all_bf16(feats)
    if not direct:
        if out_dtype == torch.bfloat16:
            raise TypeError("hop_concat: a bfloat16 result is a copy of bfloat16 hop matrices (every member of the list), nothing is rounded here")
        feats = widen_hops(feats)
    _check_hops(feats, bf16=direct)
    n, d = feats[0].shape
    H = len(feats)
    if direct:
        out, pad = _alloc_out(n, H * d, feats[0].device, dtype=out_dtype or torch.float32)
        name = "sgl_hop_concat_bf16" if out_dtype == torch.bfloat16 else "sgl_hop_concat_bf16_f32"
    else:
        out = alloc_rows(n, H * d, feats[0].device)
        name, pad = "sgl_hop_concat_padded_f32", own_pad(out)
    ptrs, lds = _lib.hop_arrays(feats)
    _call(feats[0].device, name, H, ptrs, lds, ptr(out), _ld(out), pad, n, d)
    return out


def hop_lincomb(feats, weights, outs=None):
    """out_k = sum_j weights[k, j] * feats[j]: a small dense matrix applied across the hop dimension, every input element read once
    for all outputs (sgl_hop_lincomb_f32; zero weights skipped, one fma chain in j order per output).  feats: up to 16 [n, d] hop
    matrices; weights: [n_out, len(feats)] (host or device); outs: optional list of n_out [n, d] matrices (not aliasing the inputs).
    Returns the list of outputs.  bfloat16 inputs are widened to float32 copies first (widen_hops: 4 more bytes per element of every
    hop while it runs); the outputs are float32."""
    feats = widen_hops(feats)
    _check_hops(feats)
    n, d = feats[0].shape
    w = torch.as_tensor(weights, dtype=torch.float32).to(feats[0].device).contiguous()
    if w.dim() != 2 or w.shape[1] != len(feats):
        raise ValueError("weights must be [n_out, len(feats)]")
    n_out = int(w.shape[0])
    if len(feats) > 16:
        raise ValueError("hop_lincomb takes at most 16 input matrices per call")
    if outs is None:
        outs = [alloc_rows(n, d, feats[0].device) for _ in range(n_out)]
    if len(outs) != n_out or any(tuple(o.shape) != (n, d) for o in outs):
        raise ValueError("one [n, d] output per row of weights")
    # stream whole pitches when every matrix shares one (pad columns: zeros in, zeros out)
    wide_in, _, dw = _widened(list(feats) + list(outs), outs[0])
    if dw != d:
        f_w, o_w = wide_in[:len(feats)], wide_in[len(feats):]
    else:
        f_w, o_w = list(feats), list(outs)
    ptrs, lds = _lib.hop_arrays(f_w)
    optrs, olds = _lib.hop_arrays(o_w)
    _call(feats[0].device, "sgl_hop_lincomb_f32", len(feats), ptrs, lds, n_out, optrs, olds, ptr(w), int(w.stride(0)), n, dw)
    _wrote(*outs)
    return outs


class _ReduceGrad(torch.autograd.Function):
    """sum / mean / max / min over the hop list WITH gradients (sum_message_op.py:10, mean_message_op.py:10, max_message_op.py:12,
    min_message_op.py:12): forward = the streaming reduction kernel; backward of sum = the incoming gradient broadcast to every hop,
    of mean = one true division then the broadcast, of max / min = the gradient where torch would select the hop (first NaN, else the
    first extremum), zeros elsewhere (sgl_hop_select_bwd_f32)."""

    @staticmethod
    def forward(ctx, op, divisor, *feats):
        feats_d = [f.detach() for f in feats]
        ctx.op, ctx.divisor = op, divisor
        if op == _lib.SGL_REDUCE_MEAN and divisor is not None and divisor != len(feats_d):
            # the reference divides by (end - start) whatever the slice held (mean_message_op.py:10)
            out = hop_reduce(_lib.SGL_REDUCE_SUM, feats_d)
            out = out / torch.full((), float(divisor), dtype=torch.float32, device=out.device)   # (a fill kernel, not an upload: capturable)
        else:
            out = hop_reduce(op, feats_d)
        if op in (_lib.SGL_REDUCE_MAX, _lib.SGL_REDUCE_MIN):
            ctx.save_for_backward(*feats_d)
        ctx.n_hops = len(feats_d)
        return out

    @staticmethod
    def backward(ctx, gout):
        H = ctx.n_hops
        need = [ctx.needs_input_grad[2 + h] for h in range(H)]
        if ctx.op == _lib.SGL_REDUCE_SUM:
            return (None, None, *[gout if nd else None for nd in need])
        if ctx.op == _lib.SGL_REDUCE_MEAN:
            div = float(ctx.divisor if ctx.divisor is not None else H)
            g = gout / torch.full((), div, dtype=torch.float32, device=gout.device)         # DivBackward: a true division (0-dim device divisor)
            return (None, None, *[g if nd else None for nd in need])
        feats = list(ctx.saved_tensors)
        n, d = feats[0].shape
        g = _grad_rows(gout, n, d)
        dxs = [alloc_rows(n, d, g.device) if nd else None for nd in need]
        ptrs, lds = _lib.hop_arrays(feats)
        dx_ptrs, dx_lds = _lib.hop_arrays(dxs, one_row_pitch=False)
        _call(g.device, "sgl_hop_select_bwd_f32", ctx.op, H, ptrs, lds, ptr(g), _ld(g), dx_ptrs, dx_lds, n, d)
        return (None, None, *dxs)


def hop_reduce_grad(op, feats, divisor=None):
    """hop_reduce for hop matrices that carry gradients (op: SGL_REDUCE_SUM / MEAN / MAX / MIN); bfloat16 hops are widened first
    (widen_hops)"""
    return _ReduceGrad.apply(op, divisor, *widen_hops(feats))


class _ConcatGrad(torch.autograd.Function):
    """hstack of the hop list WITH gradients (concat_message_op.py:12; the tail of ProjectedConcatMessageOp._combine,
    projected_concat_message_op.py:28): forward = hop_concat (sgl_hop_concat_padded_f32), backward = the column slices of the incoming gradient (views)."""

    @staticmethod
    def forward(ctx, *feats):
        feats_d = [f.detach() for f in feats]
        ctx.d = feats_d[0].shape[1]
        return hop_concat(feats_d)

    @staticmethod
    def backward(ctx, gout):
        d = ctx.d
        return tuple(gout[:, h * d:(h + 1) * d] if nd else None for h, nd in enumerate(ctx.needs_input_grad))


def hop_concat_grad(feats):
    return _ConcatGrad.apply(*widen_hops(feats))


class _WSum2D(torch.autograd.Function):
    """out[n,:] = sum_h W[n,h] X_h[n,:]  (two_dim_weighted_add, operators/utils.py:105-116)"""

    @staticmethod
    def forward(ctx, w, *feats):
        feats_d = [f.detach() for f in feats]
        _check_hops(feats_d)
        n, d = feats_d[0].shape
        wd = w.detach().to(torch.float32).contiguous()
        if wd.shape != (n, len(feats_d)):
            raise ValueError("The feature list and the weight list have different lengths!")
        result = alloc_rows(n, d, feats_d[0].device)
        wide, out, dw_ = _widened(feats_d, result)
        ptrs, lds = _lib.hop_arrays(wide)
        _call(out.device, "sgl_hop_wsum2d_f32", len(feats_d), ptrs, lds, ptr(wd), _ld(wd), ptr(out), _ld(out), n, dw_)
        ctx.save_for_backward(wd, *feats_d)
        return result

    @staticmethod
    def backward(ctx, gout):
        wd, *feats = ctx.saved_tensors
        H = len(feats)
        dw, dxs = _wsum2d_backward(wd, feats, gout, ctx.needs_input_grad[0], [ctx.needs_input_grad[1 + h] for h in range(H)])
        return (dw, *dxs)


def _wsum2d_backward(wd, feats, gout, need_w, need_x):
    """gradients of out = sum_h W[:, h] X_h: dW[n, h] = <dOut[n], X_h[n]> (register row-dot kernel) and dX_h = W[:, h] dOut"""
    n, d = feats[0].shape
    H = len(feats)
    g = _grad_rows(gout, n, d)
    if n > 1 and d > 4 and not rows_vectored(g) and (any(need_x) or H > 16 or d > 512):
        # autograd hands over a dense [n, d] gradient: for d % 4 != 0 its rows are not 16-byte aligned.  The dW row-dot
        # reads such a gradient directly (dword-aligned vector loads, sgl_hop_wsum2d_bwd_f32); the element-wise dX
        # kernel and the wide / many-hop fallback would drop to 4-byte lanes (0.36 of peak at d = 147), so for those
        # one copy into a padded buffer restores the 16-byte path
        gp = alloc_rows(n, d, g.device)
        gp.copy_(g)
        g = gp
    dw = torch.empty((n, H), dtype=torch.float32, device=g.device) if need_w else None
    dxs = [alloc_rows(n, d, g.device) if need_x[h] else None for h in range(H)]
    ptrs, lds = _lib.hop_arrays(feats)
    dx_ptrs, dx_lds = _lib.hop_arrays(dxs, one_row_pitch=False) if any(need_x) else (None, None)
    _call(g.device, "sgl_hop_wsum2d_bwd_f32", H, ptrs, lds, ptr(wd), _ld(wd), ptr(g), _ld(g), _opt_ptr(dw), H, dx_ptrs, dx_lds, n, d)
    return dw, dxs


def hop_wsum2d(feats, w):
    return _WSum2D.apply(w, *feats)


class _WSum1D(torch.autograd.Function):
    """out = sum_h w[h] X_h  (one_dim_weighted_add, operators/utils.py:91-102)"""

    @staticmethod
    def forward(ctx, w, *feats):
        feats_d = [f.detach() for f in feats]
        out = hop_reduce(_lib.SGL_REDUCE_WSUM, feats_d, w)
        ctx.save_for_backward(w.detach().to(torch.float32), *feats_d)
        return out

    @staticmethod
    def backward(ctx, gout):
        wd, *feats = ctx.saved_tensors
        n, d = feats[0].shape
        H = len(feats)
        g = _grad_rows(gout, n, d)
        dw = None
        if ctx.needs_input_grad[0]:
            dw = torch.empty(H, dtype=torch.float32, device=g.device)
            scratch = torch.empty(int(_call(None, "sgl_hop_wsum1d_bwd_scratch", H, raw=True)), dtype=torch.float32, device=g.device)
            ptrs, lds = _lib.hop_arrays(feats)
            _call(g.device, "sgl_hop_wsum1d_bwd_f32", H, ptrs, lds, ptr(g), _ld(g), ptr(dw), ptr(scratch), n, d)
        dxs = []
        for h in range(H):
            dxs.append(g * wd[h] if ctx.needs_input_grad[1 + h] else None)  # rarely needed: features carry no grad
        return (dw, *dxs)


def hop_wsum1d(feats, w):
    return _WSum1D.apply(w, *feats)


def hop_colsum(feats, w, shared=False):
    """[H, d] matrix of  sum_n w[n, h] * X_h[n, :]  (shared=True: w is [n], one weight per row for every hop) -- the weight
    gradient of a row-dot, X_h^T g[:, h], for all hops in ONE streaming pass (sgl_hop_colsum_f32) instead of one transposed GEMV per
    hop (rocBLAS gemvn on a padded mini-batch slice: 0.46 ms each at [50 000, 147]).  Falls back to torch where the kernel does
    not apply (rows that are not 16-byte aligned, more than 16 hops, d > 1024, CPU tensors)."""
    feats = [f.detach() for f in feats]
    H = len(feats)
    n, d = feats[0].shape
    w = w.detach().to(torch.float32)
    if (H <= 16 and 0 < d <= 1024 and n > 0 and all(f.is_cuda and f.dtype == torch.float32 and f.stride(1) == 1
                                                    and rows_vectored(f, single_row=True) for f in feats)):
        w = w.contiguous()
        out = torch.empty((H, d), dtype=torch.float32, device=feats[0].device)
        scratch = torch.empty(int(_call(None, "sgl_hop_colsum_scratch", H, n, d, raw=True)), dtype=torch.float32, device=out.device)
        ptrs, lds = _lib.hop_arrays(feats)
        _call(out.device, "sgl_hop_colsum_f32", H, ptrs, lds, ptr(w), 1 if shared else H, 0 if shared else 1, ptr(out), d, ptr(scratch), n, d)
        return out
    # products, then the column sums: a transposed matrix-vector product of the BLAS library returns NaN for a column that holds
    # one +-inf, where the sum (and sgl_hop_colsum_f32) is +-inf
    if shared:
        return torch.stack([(f * w.view(-1, 1)).sum(0) for f in feats])
    return torch.stack([(f * w[:, h:h + 1]).sum(0) for h, f in enumerate(feats)])


class _HopScores(torch.autograd.Function):
    """scores[n, h] = <X_h[n, :], v>: forward is one HIP pass over all hops; backward (mini-batch sized in training) is
    dv = sum_h X_h^T g[:, h] and dX_h = g[:, h] v^T in plain torch."""

    @staticmethod
    def forward(ctx, v, *feats):
        feats_d = [f.detach() for f in feats]
        _check_hops(feats_d)
        n, d = feats_d[0].shape
        H = len(feats_d)
        vp = _padded_vec(v, d, feats_d[0].device)
        out = torch.empty((n, H), dtype=torch.float32, device=vp.device)
        ptrs, lds = _lib.hop_arrays(feats_d)
        _call(vp.device, "sgl_hop_rowdot_f32", H, ptrs, lds, ptr(vp), ptr(out), H, n, d)
        ctx.save_for_backward(v.detach(), *feats_d)
        return out

    @staticmethod
    def backward(ctx, g):
        v, *feats = ctx.saved_tensors
        dv = None
        if ctx.needs_input_grad[0]:
            dv = hop_colsum(feats, g).sum(0).view_as(v)            # sum_h X_h^T g[:, h]: one pass over the hops
        dxs = [(g[:, h:h + 1] * v.view(1, -1)) if ctx.needs_input_grad[1 + h] else None for h in range(len(feats))]
        return (dv, *dxs)


def hop_scores(feats, v):
    """[n, H] matrix of <X_h[n, :], v> (differentiable w.r.t. v and the hops)"""
    return _HopScores.apply(v, *feats)


def _padded_vec(v, d, device, tail=None):
    """v zero-padded to whole 16-byte vectors; `tail`: one more float stored right after the padding (the gate's bias: the kernel
    reads it from there, so a bias that is a device tensor never travels to the host)"""
    dp = round_up(max(d, 1), 4)
    vp = torch.zeros(dp + (4 if tail is not None else 0), dtype=torch.float32, device=device)
    vp[:d] = v.detach().to(torch.float32).view(-1)
    if tail is not None:
        vp[dp:dp + 1] = tail.detach().to(device=device, dtype=torch.float32).reshape(-1)[:1]
    return vp


def _gate_launch(v, b, feats_d, outputs):
    """sgl_hop_gate_padded_f32 over detached hops; outputs: also write W and G [n, H] (training / return_weights) -> (out, W, G)"""
    _check_hops(feats_d)
    n, d = feats_d[0].shape
    H = len(feats_d)
    dev_ = feats_d[0].device
    vp = _padded_vec(v, d, dev_, tail=b)                  # [v | 0-pad | bias]: bias = NaN below = "read it from the device"
    result = alloc_rows(n, d, dev_)
    w, g = ((torch.empty((n, H), dtype=torch.float32, device=dev_) for _ in range(2)) if outputs else (None, None))
    ptrs, lds = _lib.hop_arrays(feats_d)
    _call(dev_, "sgl_hop_gate_padded_f32", H, ptrs, lds, ptr(vp), float("nan"), ptr(result), _ld(result), own_pad(result),
          _opt_ptr(w), H, _opt_ptr(g), H, n, d)
    return result, w, g


class _GateFused(torch.autograd.Function):
    """out = sum_h softmax_h(sigmoid(<X_h, v> + b)) X_h in ONE pass over the hops (sgl_hop_gate_padded_f32); the backward re-uses the
    dW row-dot kernel and finishes the [n, H]-sized softmax / sigmoid chain in torch."""

    @staticmethod
    def forward(ctx, v, b, *feats):
        feats_d = [f.detach() for f in feats]
        result, w, g = _gate_launch(v, b, feats_d, True)
        ctx.save_for_backward(v.detach(), w, g, *feats_d)
        ctx.b_shape = tuple(b.shape)
        ctx.mark_non_differentiable(w)
        return result, w

    @staticmethod
    def backward(ctx, gout, _gw):
        v, w, g, *feats = ctx.saved_tensors
        H = len(feats)
        need_x = [ctx.needs_input_grad[2 + h] for h in range(H)]
        dwt, dxs = _wsum2d_backward(w, feats, gout, True, need_x)                 # dL/dW and the W-part of dL/dX_h
        dg = w * (dwt - (w * dwt).sum(dim=1, keepdim=True))                       # softmax
        ds = dg * g * (1.0 - g)                                                   # sigmoid
        dv = db = None
        if ctx.needs_input_grad[0]:
            dv = hop_colsum(feats, ds).sum(0).view_as(v)           # sum_h X_h^T ds[:, h]: one pass over the hops
        if ctx.needs_input_grad[1]:
            db = ds.sum().reshape(ctx.b_shape)
        for h in range(H):
            if need_x[h]:
                dxs[h] = dxs[h] + ds[:, h:h + 1] * v.view(1, -1)
        return (dv, db, *dxs)


def gate_fusable(feats):
    """can sgl_hop_gate_padded_f32 / sgl_hop_recursive_f32 / sgl_hop_rowdot2_f32 take these hops? (register-resident rows: <= 16
    float32 hops, d <= 512, 16-byte rows)"""
    f0 = feats[0]
    return (len(feats) <= 16 and f0.is_cuda and 0 < f0.shape[1] <= 512 and f0.shape[0] > 0 and
            all(f.dtype == torch.float32 and f.stride(1) == 1 and rows_vectored(f, single_row=True) for f in feats))


def hop_gate(feats, v, b, return_weights=False):
    """LearnableWeightedMessageOp 'gate': (out, W) with W = softmax_h(sigmoid(Linear(X_h))) [n, H].  One pass over the hops
    (sgl_hop_gate_padded_f32) when their rows fit the register-resident kernel (gate_fusable); otherwise the two-pass route -- one
    row-dot pass for the scores, the [n, H] sigmoid / softmax in torch, one weighted-sum pass."""
    if gate_fusable(feats):
        if torch.is_grad_enabled() and any(t.requires_grad for t in (v, b, *feats)):
            out, w = _GateFused.apply(v, b, *feats)
        else:                                             # inference: the [n, H] matrices are written only when asked for
            out, w, _ = _gate_launch(v, b, [f.detach() for f in feats], return_weights)
    else:
        w = torch.softmax(torch.sigmoid(hop_scores(feats, v) + b.reshape(-1)[0]), dim=1)
        out = hop_wsum2d(feats, w)
    return (out, w) if return_weights else out


def recursive_weights(a, c, b):
    """The recursion of IterateLearnableWeightedMessageOp (iterate_learnable_weighted_message_op.py:35-41) on per-hop scalars:
    a[n, h] = <X_h, w_x>, c[n, h] = <X_h, w_acc>, b the Linear's bias -> the final soft-max weights [n, H].  acc is always a
    per-row weighted sum of the hops, so <acc_{i-1}, w_acc> = sum_{j<i} W[:, j] c[:, j]; plain torch, differentiable."""
    H = a.shape[1]
    dot_acc = c[:, 0]                                    # acc starts as X_0
    weights = None
    for i in range(H):
        score = torch.sigmoid(a[:, i] + dot_acc + b).unsqueeze(1)
        weights = score if weights is None else torch.hstack((weights, score))
        weights = F.softmax(weights, dim=1)              # the earlier columns are soft-maxed again (reference :39 -- kept)
        if i + 1 < H:
            dot_acc = (weights * c[:, :i + 1]).sum(dim=1)
    return weights


def _recursive_launch(weight, b, feats_d, outputs):
    """sgl_hop_recursive_f32 over detached hops; outputs: also write W, A, C [n, H] (training / return_weights) -> (out, vp, W, A, C)"""
    _check_hops(feats_d)
    n, d = feats_d[0].shape
    H = len(feats_d)
    dev_ = feats_d[0].device
    wt = weight.detach().to(device=dev_, dtype=torch.float32).reshape(-1)
    if wt.numel() != 2 * d:
        raise ValueError(f"the recursive gate's Linear has {wt.numel()} weights, the hops need 2 * {d}")
    vp = torch.cat([_padded_vec(wt[:d], d, dev_), _padded_vec(wt[d:], d, dev_, tail=b)])          # [w_x | pad | w_acc | pad | bias]
    result = alloc_rows(n, d, dev_)
    w, a, c = ((torch.empty((n, H), dtype=torch.float32, device=dev_) for _ in range(3)) if outputs else (None, None, None))
    ptrs, lds = _lib.hop_arrays(feats_d)
    # bias = NaN: "read it from the device, after the two padded vectors" (no host synchronisation on a parameter)
    _call(dev_, "sgl_hop_recursive_f32", H, ptrs, lds, ptr(vp), float("nan"), ptr(result), _ld(result), own_pad(result),
          _opt_ptr(w), H, _opt_ptr(a), H, _opt_ptr(c), H, n, d)
    return result, vp, w, a, c


class _RecursiveFused(torch.autograd.Function):
    """GAMLP-R's recursive gate in ONE pass over the hops (sgl_hop_recursive_f32): out, final weights W [n, H] and the score
    matrices A, C.  Backward: dL/dW by the row-dot kernel, the [n, H] recursion backwards in one thread-per-row kernel
    (sgl_hop_recursive_bwd_f32), the weight gradients by the column-sum kernel."""

    @staticmethod
    def forward(ctx, weight, b, *feats):
        feats_d = [f.detach() for f in feats]
        result, vp, w, a, c = _recursive_launch(weight, b, feats_d, True)
        ctx.save_for_backward(vp, w, a, c, *feats_d)
        ctx.shapes = (tuple(weight.shape), tuple(b.shape))
        ctx.mark_non_differentiable(w)
        return result, w

    @staticmethod
    def backward(ctx, gout, _gw):
        vp, w, a, c, *feats = ctx.saved_tensors
        H = len(feats)
        n, d = feats[0].shape
        dp = round_up(d, 4)
        need_x = [ctx.needs_input_grad[2 + h] for h in range(H)]
        dwt, dxs = _wsum2d_backward(w, feats, gout, True, need_x)                 # dL/dW and the W-part of dL/dX_h
        dwt = dwt.contiguous()
        da, dc = torch.empty_like(a), torch.empty_like(c)
        dbr = torch.empty(n, dtype=torch.float32, device=a.device)
        _call(a.device, "sgl_hop_recursive_bwd_f32", H, ptr(a), H, ptr(c), H, float("nan"), ptr(vp[2 * dp:]), ptr(dwt), H, ptr(da), H,
              ptr(dc), H, ptr(dbr), n)
        dweight = dbias = None
        if ctx.needs_input_grad[0]:
            dweight = torch.cat([hop_colsum(feats, da).sum(0), hop_colsum(feats, dc).sum(0)]).reshape(ctx.shapes[0])
        if ctx.needs_input_grad[1]:
            dbias = dbr.sum().reshape(ctx.shapes[1])
        v_x, v_acc = vp[:d].view(1, -1), vp[dp:dp + d].view(1, -1)
        for h in range(H):
            if need_x[h]:
                dxs[h] = dxs[h] + da[:, h:h + 1] * v_x + dc[:, h:h + 1] * v_acc
        return (dweight, dbias, *dxs)


def hop_recursive(feats, weight, b, return_weights=False):
    """IterateLearnableWeightedMessageOp 'recursive' over hops 0 .. H-1 with Linear(2 d -> 1) parameters (weight [1, 2 d] or
    [2 d]: [w_x | w_acc], bias b).  One pass over the hops when the rows fit the register-resident kernel (gate_fusable);
    otherwise two row-dot passes for the scores, the [n, H] recursion in torch and one weighted-sum pass."""
    if gate_fusable(feats):
        if torch.is_grad_enabled() and any(t.requires_grad for t in (weight, b, *feats)):
            out, w = _RecursiveFused.apply(weight, b, *feats)
        else:                                             # inference: the [n, H] matrices are written only when asked for
            out, _, w, _, _ = _recursive_launch(weight, b, [f.detach() for f in feats], return_weights)
    else:
        d = feats[0].shape[1]
        wt = weight.reshape(-1)
        w = recursive_weights(hop_scores(feats, wt[:d]), hop_scores(feats, wt[d:]), b.reshape(-1)[:1])
        out = hop_wsum2d(feats, w)
    return (out, w) if return_weights else out


class _HopScores2(torch.autograd.Function):
    """P[n, h - h0] = <X_h[n], v> for h in [h0, h1) and A[n] = sum_{j in ref} <X_j[n], U[j]>: the two parts of the 'ori_ref' /
    'jk' Linear([ref || x_h]) in one pass over the hop list (sgl_hop_rowdot2_f32).  Backward in plain torch (mini-batch sized)."""

    @staticmethod
    def forward(ctx, v, u, mask, h0, h1, *feats):
        feats_d = [f.detach() for f in feats]
        _check_hops(feats_d)
        n, d = feats_d[0].shape
        L = len(feats_d)
        dev_ = feats_d[0].device
        vp = _padded_vec(v, d, dev_)
        ldu = round_up(d, 4)
        up = torch.zeros((L, ldu), dtype=torch.float32, device=dev_)
        up[:, :d] = u.detach().to(torch.float32).view(L, d)
        p = torch.empty((n, h1 - h0), dtype=torch.float32, device=dev_)
        a = torch.empty(n, dtype=torch.float32, device=dev_)
        ptrs, lds = _lib.hop_arrays(feats_d)
        _call(dev_, "sgl_hop_rowdot2_f32", L, ptrs, lds, ptr(up), ldu, ctypes.c_uint64(mask), ptr(vp), h0, h1, ptr(p), h1 - h0, ptr(a), n, d)
        ctx.save_for_backward(v.detach(), u.detach(), *feats_d)
        ctx.meta = (mask, h0, h1)
        return p, a

    @staticmethod
    def backward(ctx, gp, ga):
        v, u, *feats = ctx.saved_tensors
        mask, h0, h1 = ctx.meta
        L = len(feats)
        d = feats[0].shape[1]
        dv = du = None
        if ctx.needs_input_grad[0]:
            dv = (hop_colsum(feats[h0:h1], gp).sum(0) if h1 > h0 else torch.zeros(d, dtype=torch.float32, device=gp.device)).view_as(v)
        if ctx.needs_input_grad[1]:
            du = torch.zeros((L, d), dtype=torch.float32, device=gp.device)
            ref = [j for j in range(L) if (mask >> j) & 1]
            if ref:                                                    # X_j^T ga for every hop of the reference part: one pass
                part = hop_colsum([feats[j] for j in ref], ga, shared=True)
                for k_, j in enumerate(ref):                           # (row by row: a list index would be uploaded, which a
                    du[j] = part[k_]                                   # HIP-graph capture of the training step does not allow)
            du = du.view_as(u)
        dxs = []
        uu = u.view(L, d)
        for j in range(L):
            if not ctx.needs_input_grad[5 + j]:
                dxs.append(None)
                continue
            gx = torch.zeros_like(feats[j])
            if h0 <= j < h1:
                gx = gx + gp[:, j - h0:j - h0 + 1] * v.view(1, -1)
            if (mask >> j) & 1:
                gx = gx + ga.view(-1, 1) * uu[j].view(1, -1)
            dxs.append(gx)
        return (dv, du, None, None, None, *dxs)


def hop_scores2(feats, v, u, mask, h0, h1):
    """(P [n, h1 - h0], A [n]): per-hop scores <X_h, v> of the adopted hops and the shared reference term sum_j <X_j, U[j]>"""
    return _HopScores2.apply(v, u, int(mask), int(h0), int(h1), *feats)


def nafs_aggregate(feats, return_weights=False):
    """OverSmoothDistanceWeightedOp._combine (over_smooth_distance_op.py:11-33) on device -> float32.  A list of bfloat16 hops is
    read in place by the register-resident kernel (sgl_nafs_bf16_f32: the float32 kernel's lane layout and arithmetic, the same
    bits as over widened copies); the shapes that kernel does not take (more than 16 hops, d > 512, rows that are not 8-byte
    aligned) and lists that mix dtypes are widened to float32 copies first (widen_hops) and go to the fp32 entry."""
    direct = _all_bf16(feats)
    if not direct:
        feats = widen_hops(feats)
    _check_hops(feats, bf16=direct)
    n, d = feats[0].shape
    H = len(feats)
    out = alloc_rows(n, d, feats[0].device)
    w = torch.empty((n, H), dtype=torch.float32, device=feats[0].device)

    def launch(name, raw=False):
        ptrs, lds = _lib.hop_arrays(feats)
        return _call(out.device, name, H, ptrs, lds, ptr(out), _ld(out), own_pad(out), ptr(w), H, n, d, raw=raw)

    rc = launch("sgl_nafs_bf16_f32", raw=True) if direct else _lib.SGL_ERR_UNSUPPORTED
    if rc == _lib.SGL_ERR_UNSUPPORTED:             # float32 hops, or not a shape of the bf16 kernel: no second bf16 kernel
        if direct:
            feats = widen_hops(feats)
        launch("sgl_nafs_padded_f32")
    else:
        check(rc, "sgl_nafs_bf16_f32")
    return (out, w) if return_weights else out


NAFS_STORE, NAFS_ADD, NAFS_ADD_DIV, NAFS_MAX = 0, 1, 2, 3


def nafs_prefix(feats, emit_hops, outs=None, combine=NAFS_STORE, divisor=1.0, outs_padded=False):
    """The over-smoothing-distance aggregate (OverSmoothDistanceWeightedOp / node_clustering.py:218-241) of EVERY requested prefix
    X_0..X_h of the hop list in one pass over the hop matrices (sgl_nafs_prefix_f32): out[k] = NAFS(feats[:emit_hops[k] + 1]).
    emit_hops: increasing hop indices < len(feats).  outs: matrices from alloc_rows to write / combine into (the multi-r
    ensemble: NAFS_ADD, NAFS_ADD_DIV with `divisor`, NAFS_MAX), allocated when None; any 16-byte aligned [n, d] views whose pitch
    is a multiple of 4 floats -- e.g. column slices of one wide slab (the 'concat' ensemble).  outs_padded=True declares that the
    tail of every output's pitch is its own padding (matrices from alloc_rows): it is then written as zeros so that every line of a
    row is written whole.  Returns the list of outputs.  bfloat16 hops are widened to float32 copies first (widen_hops: 4 more
    bytes per element of every hop while it runs)."""
    feats = widen_hops(feats)
    _check_hops(feats)
    n, d = feats[0].shape
    emit_hops = [int(h) for h in emit_hops]
    if not emit_hops or any(b <= a for a, b in zip(emit_hops, emit_hops[1:])) or emit_hops[0] < 0 or emit_hops[-1] >= len(feats):
        raise ValueError("emit_hops must be increasing hop indices below len(feats)")
    feats = feats[:emit_hops[-1] + 1]
    if outs is None:
        if combine != NAFS_STORE:
            raise ValueError("combining needs the matrices to combine with")
        outs = [alloc_rows(n, d, feats[0].device) for _ in emit_hops]
        outs_padded = True
    if len(outs) != len(emit_hops) or any(tuple(o.shape) != (n, d) or o.dtype != torch.float32 or o.device != feats[0].device for o in outs):
        raise ValueError("one [n, d] float32 output per requested prefix")
    pads = {own_pad(o) for o in outs} if outs_padded else {0}
    pad = pads.pop() if len(pads) == 1 else 0
    mask = 0
    for h in emit_hops:
        mask |= 1 << h
    ptrs, lds = _lib.hop_arrays(feats)
    optrs, olds = _lib.hop_arrays(outs)
    _call(feats[0].device, "sgl_nafs_prefix_f32", len(feats), ptrs, lds, mask, optrs, olds, pad, int(combine), float(divisor), n, d)
    _wrote(*outs)
    return outs


def scatter_rows(x, src, dst, out):
    """out[dst[i]] = x[src[i]] on device (sgl_scatter_rows_f32; src, dst: int64 CUDA tensors of one length, dst entries distinct).
    The pack step of the need-aware exchange: pairs sorted by source row, so a row several peers gather is read once."""
    _check_mat(x, "x")
    _check_mat(out, "out")
    if x.shape[1] != out.shape[1]:
        raise ValueError("scatter_rows: x and out must have the same row length")
    for t, nm in ((src, "src"), (dst, "dst")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous()):
            raise TypeError(f"scatter_rows: {nm} must be a contiguous 1-D int64 CUDA tensor")
    if src.numel() != dst.numel():
        raise ValueError("scatter_rows: src and dst must have the same length")
    if src.numel() == 0:
        return out
    _call(x.device, "sgl_scatter_rows_f32", ptr(x), _ld(x), x.shape[0], ptr(src), ptr(dst), src.numel(), ptr(out), _ld(out), out.shape[0],
          x.shape[1])
    _wrote(out)
    return out


def _device_index(idx, n_rows, device):
    """row indices of any kind as a flat int64 tensor on `device`"""
    if not (torch.is_tensor(idx) and idx.is_cuda):
        # host indices (range / list / ndarray / CPU tensor): validate here, like torch's CPU indexing does
        if isinstance(idx, range):
            idx = np.arange(idx.start, idx.stop, idx.step, dtype=np.int64)
        host = idx.numpy() if torch.is_tensor(idx) else np.asarray(idx)
        if host.dtype == np.bool_:
            host = np.nonzero(host)[0]
        host = host.astype(np.int64, copy=False).reshape(-1)
        if host.size and (host.min() < -n_rows or host.max() >= n_rows):
            raise IndexError("index out of range in row gather")
        idx = torch.from_numpy(np.ascontiguousarray(host))
    # device indices are range-checked inside the kernel (it traps on a bad index): no host round trip
    return idx.to(device=device, dtype=torch.int64).contiguous().view(-1)


def column_signature(x):
    """per-column content signatures of a [n, d] float32 device matrix with 16-byte rows (sgl_col_signature_f32): an int64 device
    tensor of round_up(d, 4) entries (the bits of the 64-bit sums), or None when the rows are not 16-byte vectors of a pitch that
    covers round_up(d, 4) columns.  Two matrices of one shape differ in column c (almost surely) iff their signatures differ at c."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        return None
    n, d = x.shape
    dw = round_up(d, 4)
    if n == 0 or d == 0:
        return None
    if x.stride(1) != 1 or not rows_vectored(x, single_row=True, width=dw, room=True):
        return None
    sig = torch.empty(dw, dtype=torch.int64, device=x.device)
    _call(x.device, "sgl_col_signature_f32", ptr(x), _ld(x, one_row=dw), n, d, ptr(sig))
    return sig


def gather_hops(feats, idx, one_launch=None):
    """[x[idx] for x in feats]: the training feed of the learnable aggregators, `[feat[idx].to(device) for feat in
    self._processed_feat_list]` (sgl/models/base_model.py:58-60), with the indices validated and uploaded ONCE for all hop
    matrices.  Host indices (what the reference's tasks pass) are where the time of the hop-by-hop form goes: 200 000 rows of 4 /
    6 / 11 hop matrices 0.46 / 0.78 / 1.25 ms -> 0.24 / 0.42 / 0.55 ms; with device indices the H queued launches already run back
    to back, and one launch over all hops (measured: profiles/r05_gather_hops.txt) is no faster."""
    feats = list(feats)
    if not feats:
        return []
    _check_mat(feats[0], "feat_list[0]", bf16=True)
    if feats[0].dtype == torch.bfloat16:
        # bf16 hop storage: the gathered rows come back as float32 (widened exactly), one launch for all hops
        for i, f in enumerate(feats):
            _check_mat(f, f"feat_list[{i}]", bf16=True)
            if f.dtype != torch.bfloat16 or f.shape != feats[0].shape or f.device != feats[0].device:
                raise ValueError("gather_hops: bfloat16 hop matrices must all be bfloat16, of one shape, on one device")
        return _gather(feats, _device_index(idx, feats[0].shape[0], feats[0].device))
    same_rows = all(torch.is_tensor(f) and f.is_cuda and f.dim() == 2 and f.shape[0] == feats[0].shape[0] and f.device == feats[0].device
                    for f in feats)
    if same_rows:
        idx = _device_index(idx, feats[0].shape[0], feats[0].device)
    one = _gather_hops_one_launch(feats, idx) if (same_rows and one_launch is not False and len(feats) > 1) else None
    if one is not None:
        return one
    return [gather_rows(x, idx) for x in feats]


def _gather_hops_one_launch(feats, idx):
    """sgl_gather_hops_padded_f32 when every hop matrix is a float32 [n, d] matrix of 16-byte rows (what propagate() returns), else None"""
    n_rows, d = feats[0].shape
    if idx.numel() < 2 or n_rows < 2 or len(feats) > 16:
        return None
    if not all(x.dtype == torch.float32 and x.shape == (n_rows, d) and x.stride(1) == 1 for x in feats):
        return None
    return _gather(feats, idx, hops_entry=True)


def _gather(feats, idx, outs=None, hops_entry=False):
    """[x[idx] as float32 for x in feats] for matrices of ONE dtype, shape and device; idx from _device_index.  outs: the caller's
    destinations, else padded float32 buffers of our own whose pad columns the kernel writes as zeros (own_out_pad).
    bfloat16 rows (sgl_gather_rows_bf16_f32 / sgl_gather_hops_bf16_f32, 16 hops per launch) are widened exactly, whatever their layout.
    float32 rows (sgl_gather_rows_padded_f32 / sgl_gather_hops_padded_f32) use 16-byte lanes for any d when source and destination
    rows are 16-byte vectors: the vector that straddles column d is READ from the source (its pitch covers it, and the storage must
    hold it for the last row too) but only the d data columns reach the result; the pad columns that get written are written as
    zeros -- never the source's tail, which may be real data when x is a column view of a wider matrix.  A caller's output is padded
    up to the next multiple of 4 only.  Several float32 hops whose rows are not such vectors: None (the caller gathers hop by hop).
    hops_entry: a single matrix goes to the many-hop entry point too (what _gather_hops_one_launch has always launched)."""
    bf16 = feats[0].dtype == torch.bfloat16
    n_rows, d = feats[0].shape
    m, dp, device = int(idx.numel()), round_up(d, 4), feats[0].device
    own = outs is None
    if own:
        outs = [alloc_rows(m, d, device, zero_pad=False) for _ in feats]
    vec = (not bf16 and m > 1 and all(rows_vectored(x, width=dp, room=True) for x in feats)
           and all(rows_vectored(o, width=dp) for o in outs))
    if not (bf16 or vec or (len(feats) == 1 and not hops_entry)):
        return None
    pad = 0
    if own:                      # the pitch's tail is ours: the kernel zeroes what it is told about, the rest is zeroed here
        ldo = outs[0].stride(0)
        if (m > 1) if bf16 else vec:
            pad = own_out_pad(ldo, d)
        if pad != ldo - d:
            for o in outs:
                padded_parent(o)[:, d + pad:].zero_()
    elif vec:
        pad = dp - d
    if m == 0 or (bf16 and d == 0):
        return outs
    for a in range(0, len(feats), 16):
        fs, os_ = feats[a:a + 16], outs[a:a + 16]
        if len(fs) == 1 and not hops_entry:
            _call(device, "sgl_gather_rows_bf16_f32" if bf16 else "sgl_gather_rows_padded_f32", ptr(fs[0]), _ld(fs[0]), n_rows, ptr(idx), m,
                  ptr(os_[0]), _ld(os_[0]), d, pad)
        else:
            ptrs, lds = _lib.hop_arrays(fs)
            optrs, olds = _lib.hop_arrays(os_)
            _call(device, "sgl_gather_hops_bf16_f32" if bf16 else "sgl_gather_hops_padded_f32", len(fs), ptrs, lds, n_rows, ptr(idx), m,
                  optrs, olds, d, pad)
    _wrote(*outs)
    return outs


def _device_edges(edges, n_a, n_b, device):
    """an edge list of any kind as a contiguous int64 [E, 2] tensor on `device`.  `edges`: an [E, 2] tensor / ndarray (host or
    device), or a pair (u, v) -- a tuple or list of two index sequences of one length (a Python list of two is always read as that
    pair).  Host indices are validated here, column 0 against n_a and column 1 against n_b, as _device_index does; device index
    tensors are not (the kernel turns a bad pair into NaN)."""
    if isinstance(edges, (tuple, list)) and len(edges) == 2:
        u, v = edges
        if torch.is_tensor(u) and torch.is_tensor(v) and u.is_cuda and v.is_cuda:
            if u.dim() != 1 or u.shape != v.shape:
                raise ValueError("edge_dot: u and v must be 1-D and of one length")
            return torch.stack((u.to(device=device, dtype=torch.int64), v.to(device=device, dtype=torch.int64)), dim=1).contiguous()
        u, v = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (u, v))
        if u.ndim != 1 or u.shape != v.shape:
            raise ValueError("edge_dot: u and v must be 1-D and of one length")
        edges = np.stack((u.astype(np.int64, copy=False), v.astype(np.int64, copy=False)), axis=1) if u.size else np.zeros((0, 2), np.int64)
    if not (torch.is_tensor(edges) and edges.is_cuda):
        host = edges.numpy() if torch.is_tensor(edges) else np.asarray(edges)
        if host.size == 0:
            host = host.reshape(0, 2)
        if host.ndim != 2 or host.shape[1] != 2:
            raise ValueError("edge_dot: edges must be [E, 2] (or a pair (u, v))")
        if host.dtype.kind not in "iu":
            raise TypeError("edge_dot: edges must be integers")
        host = host.astype(np.int64, copy=False)
        if host.shape[0] and (host[:, 0].min() < -n_a or host[:, 0].max() >= n_a or host[:, 1].min() < -n_b or host[:, 1].max() >= n_b):
            raise IndexError("index out of range in edge list")
        edges = torch.from_numpy(np.ascontiguousarray(host))
    elif edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("edge_dot: edges must be [E, 2] (or a pair (u, v))")
    return edges.to(device=device, dtype=torch.int64).contiguous()


EDGE_DOT_MAX_EDGES = 1 << 27          # edges per launch (every lane layout's grid fits one launch); longer lists are split


def edge_dot(a, b, edges, out=None):
    """out[e] = <a[u_e], b[v_e]> for the pairs of `edges` (sgl_edge_dot_f32): the entries `torch.mm(a, b.t())[u, v]` of the reference's
    link-prediction scores (tasks/link_prediction.py:282-283, tasks/utils.py:281-285) without the [n_a, n_b] matrix.
    a, b: [n_a, d] / [n_b, d] float32 CUDA matrices (b may be a; padded buffers and column views are read in place); edges: see
    _device_edges.  Negative indices count from the end; in a DEVICE index tensor a pair outside the matrices gives NaN for that edge
    (host indices raise IndexError).  Returns / fills a float32 [E] tensor.  Lists too long for one launch are split: edges are
    independent, the bits do not change."""
    _no_bf16("edge_dot", a, b)
    _check_mat(a, "a")
    _check_mat(b, "b")
    if a.shape[1] != b.shape[1] or a.device != b.device:
        raise ValueError("edge_dot: a and b must have the same row length and live on one device")
    d = a.shape[1]
    edges = _device_edges(edges, a.shape[0], b.shape[0], a.device)
    n_e = edges.shape[0]
    if out is None:
        out = torch.empty(n_e, dtype=torch.float32, device=a.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == a.device and out.dtype == torch.float32 and out.dim() == 1
              and out.numel() == n_e and out.is_contiguous()):
        raise ValueError("edge_dot: `out` must be a contiguous float32 [E] tensor on the matrices' device")
    _split_calls("sgl_edge_dot_f32", n_e,
                 lambda lo, m: _call(a.device, "sgl_edge_dot_f32", ptr(a), _ld(a), a.shape[0], ptr(b), _ld(b), b.shape[0],
                                     c_void_p(edges.data_ptr() + 16 * lo), m, d, c_void_p(out.data_ptr() + 4 * lo), raw=True))
    _wrote(out)
    return out


def _split_calls(name, n_items, one):
    """edge_dot's list splitting for an entry point whose items are independent: `one(lo, m)` makes the call for the items
    [lo, lo + m) and returns its unchecked code; a piece more than one launch covers (SGL_ERR_UNSUPPORTED) is halved."""
    step, lo = max(int(EDGE_DOT_MAX_EDGES), 1), 0
    while lo < n_items:
        m = min(step, n_items - lo)
        rc = one(lo, m)
        if rc == _lib.SGL_ERR_UNSUPPORTED and m > 1:
            step = (m + 1) // 2
            continue
        check(rc, name)
        lo += m


# ---- the prepared edge list of the link-prediction training step (sgl_edge_loss_grad_f32; tricks.link_prediction.EdgePlan) ------------
EDGE_LOSS_MODES = {"sigmoid": 0, "none": 1, "given": 2}      # SIGMOID_LOGITS (the reference as written), LOGITS, GIVEN
EDGE_LOSS_MAX_PIECE = 128             # incidences per piece: the fastest of 128 ... 4096, uncut (profiles/edge_loss.log); max_piece=None means this


def edge_incidence(u, v, n):
    """(inc_ptr int64 [n + 1], inc_other int32 [2 E], inc_edge int64 [2 E]): the edges (u_e, v_e) grouped by node, on the device u
    and v are on (CPU included; index arithmetic in torch only).  Entry k of node i's range [inc_ptr[i], inc_ptr[i + 1]) joins i and
    inc_other[k] through edge e: inc_edge[k] = e when i is u_e (the primary entry), ~e when i is v_e.  Inside a range the entries
    ascend by e; a self pair (i, i) has both entries in i's range, primary first; duplicates stay separate.  u, v: int64 [E], every
    index in [0, n)."""
    e = int(u.numel())
    rows = torch.stack((u, v), dim=1).reshape(-1)                                   # entry 2 e: u_e, entry 2 e + 1: v_e
    rows, order = torch.sort(rows, stable=True)                                     # stable: ascending e, primary first
    ids = torch.arange(e, dtype=torch.int64, device=u.device)
    inc_edge = torch.stack((ids, ~ids), dim=1).reshape(-1)[order]
    inc_other = torch.stack((v, u), dim=1).reshape(-1)[order].to(torch.int32)
    inc_ptr = torch.zeros(n + 1, dtype=torch.int64, device=u.device)
    torch.cumsum(torch.bincount(rows, minlength=n), 0, out=inc_ptr[1:])
    return inc_ptr, inc_other.contiguous(), inc_edge.contiguous()


def edge_pieces(inc_ptr, max_piece):
    """(pieces int64 [P, 4], fold int64 [F, 3], n_partial) for the ranges of inc_ptr cut into pieces of at most max_piece entries.
    pieces[p] = (row, begin, end, dest), in row order and inside a row in entry order: dest = -1 for a row that is one piece (it
    writes dZ[row]; a row without entries has one empty piece), else the row of the partial buffer the piece writes.  fold[f] =
    (row, first, count) for every cut row: its partial rows are first .. first + count - 1, in piece order."""
    n = int(inc_ptr.numel()) - 1
    dv = inc_ptr.device
    max_piece = int(max_piece)
    if max_piece < 1:
        raise ValueError("max_piece must be at least 1")
    deg = inc_ptr[1:] - inc_ptr[:-1]
    per_row = torch.clamp((deg + (max_piece - 1)) // max_piece, min=1)
    first_piece = torch.cumsum(per_row, 0) - per_row
    row = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dv), per_row)
    n_pieces = int(row.numel())
    begin = inc_ptr[:-1][row] + (torch.arange(n_pieces, dtype=torch.int64, device=dv) - first_piece[row]) * max_piece
    end = torch.minimum(begin + max_piece, inc_ptr[1:][row])
    cut = per_row[row] > 1
    dest = torch.where(cut, torch.cumsum(cut.to(torch.int64), 0) - 1, torch.full_like(row, -1))
    pieces = torch.stack((row, begin, end, dest), dim=1).contiguous()
    cut_rows = torch.nonzero(per_row > 1).reshape(-1)
    count = per_row[cut_rows]
    fold = torch.stack((cut_rows, torch.cumsum(count, 0) - count, count), dim=1).contiguous()
    return pieces, fold, int(count.sum()) if cut_rows.numel() else 0


def edge_loss_grad(z, plan, mode, w=1.0, given=None, dz=None, score=None, coef=None):
    """One launch of sgl_edge_loss_grad_f32 over the prepared edge list `plan` (anything with EdgePlan's tables): dz [n, d] is
    OVERWRITTEN with sum over the edges at i of c_e z_j -- a node without edges gets exact zeros -- and the piece losses land in
    plan.piece_loss.  mode: a key of EDGE_LOSS_MODES; "given": c_e = given[e], nothing else is computed.  score / coef: optional
    float32 [E] outputs (the logits of dev.edge_dot, bit for bit, and the coefficients).  Returns dz (allocated when None).  Nothing
    here synchronises; a piece table longer than one launch covers is split (pieces are independent, the fold runs last)."""
    _no_bf16("edge_loss_grad", z)
    _check_mat(z, "z")
    n, d = z.shape
    if n != plan.n:
        raise ValueError(f"edge_loss_grad: z has {n} rows, the plan was built for {plan.n} nodes")
    if plan.pieces.device != z.device:
        raise ValueError("edge_loss_grad: the plan and z must live on one device")
    m = EDGE_LOSS_MODES[mode]
    n_e = plan.n_edges

    def vector(t, name):
        if t is None:
            return None
        if not (torch.is_tensor(t) and t.device == z.device and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == n_e
                and t.is_contiguous()):
            raise ValueError(f"edge_loss_grad: `{name}` must be a contiguous float32 [E] tensor on z's device")
        return t

    given, score, coef = vector(given, "given"), vector(score, "score"), vector(coef, "coef")
    if (mode == "given") != (given is not None) or (mode == "given" and (score is not None or coef is not None)):
        raise ValueError("edge_loss_grad: `given` goes with mode 'given' alone, which has no score or coef output")
    if dz is None:
        dz = alloc_rows(n, d, z.device)
    else:
        _check_mat(dz, "dz")
        if dz.shape != z.shape or dz.device != z.device:
            raise ValueError("edge_loss_grad: `dz` must have z's shape and device")
    if n_e == 0 or d == 0:                              # no edges: dZ = 0 and no loss; no columns: every score is an empty sum
        dz.zero_()
        plan.piece_loss.zero_()
        for t in (score, coef):
            if t is not None:
                t.zero_()
        return dz
    partial = plan.partial_rows(d)
    pieces, fold = plan.pieces, plan.fold
    n_p, n_f = pieces.shape[0], fold.shape[0]
    loss = None if mode == "given" else plan.piece_loss

    def one(lo, cnt):
        last = lo + cnt == n_p
        return _call(z.device, "sgl_edge_loss_grad_f32", ptr(z), _ld(z), n, d, c_void_p(pieces.data_ptr() + 32 * lo), cnt,
                     ptr(plan.inc_other), ptr(plan.inc_edge), 2 * n_e, ptr(plan.labels), _opt_ptr(given), n_e, m, float(w), ptr(dz),
                     _ld(dz), _opt_ptr(partial), _ld(partial) if partial is not None else 0, plan.n_partial,
                     ptr(fold) if (last and n_f) else None, n_f if last else 0, _opt_ptr(score), _opt_ptr(coef),
                     c_void_p(loss.data_ptr() + 4 * lo) if loss is not None else None, raw=True)

    _split_calls("sgl_edge_loss_grad_f32", n_p, one)
    _wrote(dz, score, coef, loss)
    return dz


def _csr_arrays(adj, who):
    """(rowptr, col) of a device CSR (DeviceAdjacency or anything with its fields) as the two search entries take them; a matrix
    without entries gets one unread column slot, so that the pointer is never NULL"""
    rowptr, col = adj.rowptr, adj.col
    if not (torch.is_tensor(rowptr) and rowptr.is_cuda and rowptr.dtype == torch.int64 and rowptr.is_contiguous()
            and rowptr.numel() == adj.shape[0] + 1):
        raise TypeError(f"{who}: adj.rowptr must be a contiguous int64 CUDA tensor of n_rows + 1 offsets")
    if not (torch.is_tensor(col) and col.device == rowptr.device and col.dtype == torch.int32 and col.is_contiguous()):
        raise TypeError(f"{who}: adj.col must be a contiguous int32 tensor on the device of adj.rowptr")
    if col.numel() == 0:
        col = torch.zeros(1, dtype=torch.int32, device=rowptr.device)
    return rowptr, col


def csr_find(adj, edges):
    """pos[q] = where the pair edges[q] = (u, v) is stored in the canonical device CSR `adj` (a DeviceAdjacency: columns sorted and
    unique inside each row): the p in [rowptr[u], rowptr[u + 1]) with col[p] == v, or -1 (sgl_csr_find: a search inside one row per
    pair).  edges: see _device_edges.  Negative indices count from the end; in a DEVICE index tensor a pair outside the matrix gives
    -1 (host indices raise IndexError).  Returns an int64 [Q] tensor.  Lists too long for one launch are split."""
    rowptr, col = _csr_arrays(adj, "csr_find")
    n_rows, n_cols = adj.shape
    edges = _device_edges(edges, n_rows, n_cols, rowptr.device)
    pos = torch.empty(edges.shape[0], dtype=torch.int64, device=rowptr.device)
    _split_calls("sgl_csr_find", edges.shape[0],
                 lambda lo, m: _call(rowptr.device, "sgl_csr_find", ptr(rowptr), ptr(col), n_rows, n_cols, c_void_p(edges.data_ptr() + 16 * lo), m,
                                     c_void_p(pos.data_ptr() + 8 * lo), raw=True))
    _wrote(pos)
    return pos


def edge_candidates(adj, seed, first, count):
    """(edges int64 [count, 2], key int64 [count]) for the candidates first .. first + count - 1 of the seeded stream of ordered pairs
    over the square canonical device CSR `adj` (sgl_edge_candidates): key = min(i, j) * n + max(i, j) when i != j and (i, j) is not
    stored, else -1.  A candidate depends on (seed, its number) alone, so ranges can be drawn in any pieces."""
    rowptr, col = _csr_arrays(adj, "edge_candidates")
    n = adj.shape[0]
    first, count = int(first), int(count)
    if adj.shape[1] != n or n < 1:
        raise ValueError("edge_candidates: adj must be square with at least one node")
    if first < 0 or count < 0:
        raise ValueError("edge_candidates: first and count must not be negative")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    edges = torch.empty((count, 2), dtype=torch.int64, device=rowptr.device)
    key = torch.empty(count, dtype=torch.int64, device=rowptr.device)
    _split_calls("sgl_edge_candidates", count,
                 lambda lo, m: _call(rowptr.device, "sgl_edge_candidates", ptr(rowptr), ptr(col), n, seed, first + lo, m,
                                     c_void_p(edges.data_ptr() + 16 * lo), c_void_p(key.data_ptr() + 8 * lo), raw=True))
    _wrote(edges, key)
    return edges, key


CSR_SELECT_LANES = (4, 16, 64)       # the compiled lanes-per-row instances of csr_select_kernel (sgl_csr_select.hip)


def csr_select(adj, row_map=None, col_map=None, n_rows_out=None, n_cols_out=None, entry_keep=None, symmetric_mask=False, drop_self=False,
               drop_below=0, seed=0, symmetric=False, lanes=0, positions=False):
    """A canonical device CSR filtered into a new one (sgl_csr_select_rowptr + sgl_csr_select_fill; include/sgl_hip.h states the
    predicate): entry p = (i, j, v) is kept iff row_map[i] and col_map[j] are new ids (int32 [n] device tensors, -1 = dropped, None =
    identity; kept ids must increase with the old id), entry_keep[p] is set (uint8 / bool [nnz], None = all; with symmetric_mask the
    flag of the pair's upper entry decides both directions), not (drop_self and i == j), and h(seed, 103, i, j) >= drop_below (with
    symmetric: h of (min, max)).  Returns a DeviceAdjacency of shape (n_rows_out, n_cols_out) -- defaults: adj's when the map is None --
    and, with positions=True, also the int64 position in adj of every kept entry.  lanes: 0 = auto, or one of CSR_SELECT_LANES.
    The first call synchronises the device (the size of the result comes back through the host and its scratch is freed with hipFree)."""
    from .io import DeviceAdjacency
    rowptr, col = _csr_arrays(adj, "csr_select")
    val = adj.val
    dv = rowptr.device
    n_rows, n_cols = adj.shape
    nnz = int(adj.col.numel())
    if not (torch.is_tensor(val) and val.device == dv and val.dtype == torch.float32 and val.is_contiguous() and val.numel() == nnz):
        raise TypeError("csr_select: adj.val must be a contiguous float32 tensor of nnz values on the device of adj.rowptr")
    if n_rows > 0 and int(rowptr[-1]) != nnz:
        raise ValueError(f"csr_select: adj.rowptr ends at {int(rowptr[-1])}, adj.col holds {nnz} entries")
    if nnz == 0:
        val = torch.zeros(1, dtype=torch.float32, device=dv)

    def id_map(m, n_old, n_out, name):
        if m is None:
            if n_out is not None and int(n_out) != n_old:
                raise ValueError(f"csr_select: without `{name}` the output keeps adj's size on that side")
            return None, n_old
        if n_out is None:
            raise ValueError(f"csr_select: `{name}` needs the number of new ids")
        if not (torch.is_tensor(m) and m.device == dv and m.dtype == torch.int32 and m.dim() == 1 and m.numel() == n_old and m.is_contiguous()):
            raise ValueError(f"csr_select: `{name}` must be a contiguous int32 [{n_old}] tensor on adj's device")
        if int(n_out) < 0:
            raise ValueError("csr_select: the number of new ids must not be negative")
        return m, int(n_out)

    row_map, n_rows_out = id_map(row_map, n_rows, n_rows_out, "row_map")
    col_map, n_cols_out = id_map(col_map, n_cols, n_cols_out, "col_map")
    if entry_keep is not None:
        if not (torch.is_tensor(entry_keep) and entry_keep.device == dv and entry_keep.dtype in (torch.uint8, torch.bool)
                and entry_keep.dim() == 1 and entry_keep.numel() == nnz and entry_keep.is_contiguous()):
            raise ValueError(f"csr_select: `entry_keep` must be a contiguous uint8 or bool [{nnz}] tensor on adj's device")
        if nnz == 0:
            entry_keep = torch.zeros(1, dtype=torch.uint8, device=dv)
    elif symmetric_mask:
        raise ValueError("csr_select: symmetric_mask needs `entry_keep`")
    if symmetric_mask and n_rows != n_cols:
        raise ValueError("csr_select: symmetric_mask needs a square matrix")
    lanes = int(lanes)
    if lanes != 0 and lanes not in CSR_SELECT_LANES:
        raise ValueError(f"csr_select: lanes must be 0 (auto) or one of {CSR_SELECT_LANES}, not {lanes}")
    drop_below = int(drop_below)
    if not 0 <= drop_below < (1 << 64):
        raise ValueError("csr_select: drop_below is an unsigned 64-bit threshold")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    select = (ptr(row_map) if row_map is not None else None, ptr(col_map) if col_map is not None else None, n_rows_out, n_cols_out,
              _opt_ptr(entry_keep), int(bool(symmetric_mask)), int(bool(drop_self)), drop_below, seed, int(bool(symmetric)), lanes)
    out_rowptr = torch.empty(n_rows_out + 1, dtype=torch.int64, device=dv)
    total = c_int64(0)
    _call(dv, "sgl_csr_select_rowptr", ptr(rowptr), ptr(col), n_rows, n_cols, nnz, *select, ptr(out_rowptr), ctypes.byref(total))
    m = total.value
    out_col = torch.empty(max(m, 1), dtype=torch.int32, device=dv)
    out_val = torch.empty(max(m, 1), dtype=torch.float32, device=dv)
    out_pos = torch.empty(max(m, 1), dtype=torch.int64, device=dv) if positions else None
    _call(dv, "sgl_csr_select_fill", ptr(rowptr), ptr(col), ptr(val), n_rows, n_cols, nnz, *select, ptr(out_rowptr), ptr(out_col), ptr(out_val),
          _opt_ptr(out_pos))
    _wrote(out_rowptr, out_col, out_val, out_pos)
    out = DeviceAdjacency(out_rowptr, out_col[:m], out_val[:m], (n_rows_out, n_cols_out))
    return (out, out_pos[:m]) if positions else out


CSR_MERGE_LANES = (4, 16, 64)        # the compiled lanes-per-row instances of csr_merge_kernel (sgl_csr_merge.hip)
CSR_MERGE_MODES = {"sum": _lib.SGL_MERGE_SUM, "keep": _lib.SGL_MERGE_KEEP_A}


def csr_merge(a, b, mode="sum", lanes=0, positions=False):
    """The row-wise union of two canonical device CSRs of one shape as a new one (sgl_csr_merge_rowptr + sgl_csr_merge_fill;
    include/sgl_hip.h states the contract): every column stored in row i of `a` or of `b`, once, ascending.  A column stored on both
    sides gets a + b (one float32 addition; a zero sum stays stored) under mode="sum" and a's value under mode="keep"; a column
    stored on one side keeps that side's bits.  Returns a DeviceAdjacency and, with positions=True, also (pos_a, pos_b): the int64
    position of every output entry in `a` and in `b`, -1 where that side does not store it.  lanes: 0 = auto, or one of
    CSR_MERGE_LANES.  The first call synchronises the device (the size of the result comes back through the host and its scratch is freed with hipFree)."""
    from .io import DeviceAdjacency
    rowptr_a, col_a = _csr_arrays(a, "csr_merge")
    rowptr_b, col_b = _csr_arrays(b, "csr_merge")
    dv = rowptr_a.device
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"csr_merge: the shapes differ: {tuple(a.shape)} and {tuple(b.shape)}")
    if rowptr_b.device != dv:
        raise ValueError("csr_merge: a and b must live on one device")
    n_rows, n_cols = a.shape
    if mode not in CSR_MERGE_MODES:
        raise ValueError(f"csr_merge: mode must be one of {tuple(CSR_MERGE_MODES)}, not {mode!r}")
    lanes = int(lanes)
    if lanes != 0 and lanes not in CSR_MERGE_LANES:
        raise ValueError(f"csr_merge: lanes must be 0 (auto) or one of {CSR_MERGE_LANES}, not {lanes}")
    sides = []
    for name, adj, rowptr, col in (("a", a, rowptr_a, col_a), ("b", b, rowptr_b, col_b)):
        val = adj.val
        nnz = int(adj.col.numel())
        if not (torch.is_tensor(val) and val.device == dv and val.dtype == torch.float32 and val.is_contiguous() and val.numel() == nnz):
            raise TypeError(f"csr_merge: {name}.val must be a contiguous float32 tensor of nnz values on the device of a.rowptr")
        if n_rows > 0 and int(rowptr[-1]) != nnz:
            raise ValueError(f"csr_merge: {name}.rowptr ends at {int(rowptr[-1])}, {name}.col holds {nnz} entries")
        if nnz == 0:
            col, val = torch.zeros(1, dtype=torch.int32, device=dv), torch.zeros(1, dtype=torch.float32, device=dv)
        sides.append((rowptr, col, val, nnz))
    (ra, ca, va, na), (rb, cb, vb, nb) = sides
    out_rowptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dv)
    total = c_int64(0)
    _call(dv, "sgl_csr_merge_rowptr", ptr(ra), ptr(ca), na, ptr(rb), ptr(cb), nb, n_rows, n_cols, lanes, ptr(out_rowptr), ctypes.byref(total))
    m = total.value
    out_col = torch.empty(max(m, 1), dtype=torch.int32, device=dv)
    out_val = torch.empty(max(m, 1), dtype=torch.float32, device=dv)
    pos_a = torch.empty(max(m, 1), dtype=torch.int64, device=dv) if positions else None
    pos_b = torch.empty(max(m, 1), dtype=torch.int64, device=dv) if positions else None
    _call(dv, "sgl_csr_merge_fill", ptr(ra), ptr(ca), ptr(va), na, ptr(rb), ptr(cb), ptr(vb), nb, n_rows, n_cols, CSR_MERGE_MODES[mode], lanes,
          ptr(out_rowptr), ptr(out_col), ptr(out_val), _opt_ptr(pos_a), _opt_ptr(pos_b))
    _wrote(out_rowptr, out_col, out_val, pos_a, pos_b)
    out = DeviceAdjacency(out_rowptr, out_col[:m], out_val[:m], (n_rows, n_cols))
    return (out, (pos_a[:m], pos_b[:m])) if positions else out


def kmeans_assign(x, centres, want_dist=True):
    """(labels, mindist) of the k-means assignment step (sgl_kmeans_assign_f32): labels[i] = argmin_j |x[i] - centres[j]|^2 (int64 [n],
    the lowest index on a tie) and that minimum (float32 [n]; None with want_dist=False) -- the direct sum of squared differences, not
    the expanded form.  x: [n, d], centres: [k, d] float32 CUDA matrices on one device, read in place (padded buffers, column views).
    A row that holds NaN gets label 0 and mindist NaN.  No atomics: two runs are bit-equal."""
    _no_bf16("kmeans_assign", x, centres)
    _check_mat(x, "x")
    _check_mat(centres, "centres")
    if x.shape[1] != centres.shape[1] or x.device != centres.device:
        raise ValueError("kmeans_assign: x and centres must have the same row length and live on one device")
    n, k = x.shape[0], centres.shape[0]
    if k < 1 and n > 0:
        raise ValueError("kmeans_assign: at least one centre is needed")
    labels = torch.empty(n, dtype=torch.int64, device=x.device)
    mindist = torch.empty(n, dtype=torch.float32, device=x.device) if want_dist else None
    _call(x.device, "sgl_kmeans_assign_f32", ptr(x), _ld(x), n, x.shape[1], ptr(centres), _ld(centres), k, ptr(labels), _opt_ptr(mindist))
    return labels, mindist


def cluster_loss_grad(x, centres, labels, w, dx=None, row_loss=None):
    """One launch of sgl_cluster_loss_grad_f32: with D_ij = |x[i] - centres[j]|_2 and y_i = labels[i] (int64 [n] on x's device),
    row_loss[i] = 2 D_{i, y_i} - mean_j D_ij (float32 [n]) and dx[i] = w sum_j a_ij (x[i] - centres[j]), a_ij = (2 [j = y_i] - 1 / k) /
    D_ij and 0 where D_ij = 0 -- the direct form, differences first.  x: [n, d], centres: [k, d] float32 CUDA matrices on one device,
    read in place (padded buffers, column views).  dx / row_loss: True allocates the output, a tensor is written in place, None /
    False leaves it out; at least one is needed.  A label outside [0, k) means "no assigned centre" (nothing is indexed by it).
    Returns (dx, row_loss).  No atomics: two runs are bit-equal.  Nothing here synchronises."""
    _no_bf16("cluster_loss_grad", x, centres, dx, row_loss)
    _check_mat(x, "x")
    _check_mat(centres, "centres")
    if x.shape[1] != centres.shape[1] or x.device != centres.device:
        raise ValueError("cluster_loss_grad: x and centres must have the same row length and live on one device")
    n, d = x.shape
    k = centres.shape[0]
    if k < 1:
        raise ValueError("cluster_loss_grad: at least one centre is needed")
    if not (torch.is_tensor(labels) and labels.device == x.device and labels.dtype == torch.int64 and labels.dim() == 1
            and labels.numel() == n and labels.is_contiguous()):
        raise ValueError("cluster_loss_grad: `labels` must be a contiguous int64 [n] tensor on x's device")
    dx = None if dx is False else dx
    row_loss = None if row_loss is False else row_loss
    if dx is None and row_loss is None:
        raise ValueError("cluster_loss_grad: at least one of `dx` and `row_loss` is needed")
    if dx is True:
        dx = alloc_rows(n, d, x.device)
    elif dx is not None:
        _check_mat(dx, "dx")
        if dx.shape != x.shape or dx.device != x.device:
            raise ValueError("cluster_loss_grad: `dx` must have x's shape and device")
    if row_loss is True:
        row_loss = torch.empty(n, dtype=torch.float32, device=x.device)
    elif row_loss is not None and not (torch.is_tensor(row_loss) and row_loss.device == x.device and row_loss.dtype == torch.float32
                                       and row_loss.dim() == 1 and row_loss.numel() == n and row_loss.is_contiguous()):
        raise ValueError("cluster_loss_grad: `row_loss` must be a contiguous float32 [n] tensor on x's device")
    _call(x.device, "sgl_cluster_loss_grad_f32", ptr(x), _ld(x), n, d, ptr(centres), _ld(centres), k, ptr(labels), float(w), _opt_ptr(dx),
          _ld(dx) if dx is not None else 0, _opt_ptr(row_loss))
    _wrote(dx, row_loss)
    return dx, row_loss


def class_loss_grad(z, labels, w, dz=False, row_loss=False, pred=False):
    """One launch of sgl_class_loss_grad_f32 over the logits z [n, c]: with lse_i = log sum_j exp(z[i, j]) (the row's maximum taken out
    first) and y_i = labels[i] (int64 [n] on z's device), row i LIVE iff 0 <= y_i < c,
    row_loss[i] = lse_i - z[i, y_i] (float32 [n]), dz[i] = w (softmax(z[i]) - onehot(y_i)), both 0 for a row that is not live, and
    pred[i] = the lowest index of the row's maximum (int64 [n]; a NaN counts as the maximum, the first NaN wins).  z: a float32 CUDA
    matrix read in place (padded buffers, column views).  dz / row_loss / pred: True allocates the output, a tensor is written in
    place, None / False leaves it out; at least one is needed.  labels may be None when pred is the only output: no exp is evaluated
    then.  Returns (dz, row_loss, pred).  No atomics: two runs are bit-equal.  Nothing here synchronises."""
    _no_bf16("class_loss_grad", z, dz, row_loss)
    _check_mat(z, "z")
    n, c = z.shape
    if c < 1:
        raise ValueError("class_loss_grad: at least one class is needed")
    dz = None if dz is False else dz
    row_loss = None if row_loss is False else row_loss
    pred = None if pred is False else pred
    if dz is None and row_loss is None and pred is None:
        raise ValueError("class_loss_grad: at least one of `dz`, `row_loss` and `pred` is needed")
    if labels is None:
        if dz is not None or row_loss is not None:
            raise ValueError("class_loss_grad: `labels` may be None only when `pred` is the only output")
    elif not (torch.is_tensor(labels) and labels.device == z.device and labels.dtype == torch.int64 and labels.dim() == 1
              and labels.numel() == n and labels.is_contiguous()):
        raise ValueError("class_loss_grad: `labels` must be a contiguous int64 [n] tensor on z's device")
    if dz is True:
        dz = alloc_rows(n, c, z.device)
    elif dz is not None:
        _check_mat(dz, "dz")
        if dz.shape != z.shape or dz.device != z.device:
            raise ValueError("class_loss_grad: `dz` must have z's shape and device")
    if row_loss is True:
        row_loss = torch.empty(n, dtype=torch.float32, device=z.device)
    elif row_loss is not None and not (torch.is_tensor(row_loss) and row_loss.device == z.device and row_loss.dtype == torch.float32
                                       and row_loss.dim() == 1 and row_loss.numel() == n and row_loss.is_contiguous()):
        raise ValueError("class_loss_grad: `row_loss` must be a contiguous float32 [n] tensor on z's device")
    if pred is True:
        pred = torch.empty(n, dtype=torch.int64, device=z.device)
    elif pred is not None and not (torch.is_tensor(pred) and pred.device == z.device and pred.dtype == torch.int64 and pred.dim() == 1
                                   and pred.numel() == n and pred.is_contiguous()):
        raise ValueError("class_loss_grad: `pred` must be a contiguous int64 [n] tensor on z's device")
    _call(z.device, "sgl_class_loss_grad_f32", ptr(z), _ld(z), n, c, _opt_ptr(labels), float(w), _opt_ptr(dz),
          _ld(dz) if dz is not None else 0, _opt_ptr(row_loss), _opt_ptr(pred))
    _wrote(dz, row_loss, pred)
    return dz, row_loss, pred


def gather_rows(x, idx, out=None):
    """x[idx] on device (BaseSGAPModel.forward's per-step row gather, models/base_model.py:58,60).  `out`: optional
    preallocated [len(idx), d] destination (the pack step of the need-aware exchange re-uses one send buffer per hop).
    A bfloat16 x (bf16 hop storage) is gathered into float32 (sgl_gather_rows_bf16_f32): `out`, given or not, is float32."""
    _check_mat(x, "x", bf16=True)
    idx = _device_index(idx, x.shape[0], x.device)
    if out is not None:
        _check_mat(out, "out")
        if out.shape != (idx.numel(), x.shape[1]):
            raise ValueError("gather_rows: `out` must be [len(idx), d]")
    return _gather([x], idx, None if out is None else [out])[0]


# ---- K16: the sub-graph ensemble aggregators of the heterogeneous models (include/sgl_ensemble.h) -----------------------------------
def _ensemble_members(groups):
    """(flat member-major list, n_groups, group_size) of a list of equally long lists of [n_rows, d] float32 CUDA matrices"""
    groups = [list(g) for g in groups]
    if not groups or not groups[0] or any(len(g) != len(groups[0]) for g in groups):
        raise ValueError("ensemble_combine: `groups` must be a non-empty list of equally long, non-empty lists of matrices")
    flat = [x for g in groups for x in g]
    for i, x in enumerate(flat):
        if torch.is_tensor(x) and x.dtype == torch.bfloat16:
            raise TypeError("ensemble_combine has no bfloat16 form: the propagated matrices of the heterogeneous models are float32")
        _check_mat(x, f"groups[{i // len(groups[0])}][{i % len(groups[0])}]")
        if x.requires_grad:
            raise TypeError("ensemble_combine: the matrices are constants of the model (there is no dX); detach them")
        if x.shape != flat[0].shape or x.device != flat[0].device:
            raise ValueError("ensemble_combine: all matrices must have the same shape and device")
    return flat, len(groups), len(groups[0])


def _ensemble_weight_mode(weights, m_total, d):
    """cs of a member-major weight table: 1 for [M, d] (one weight per matrix and column), 0 for [M] / [M, 1] (one per matrix)"""
    if not (torch.is_tensor(weights) and weights.is_floating_point()):
        raise TypeError("ensemble_combine: `weights` must be a floating-point tensor")
    if weights.dim() == 1 and weights.shape[0] == m_total:
        return 0
    if weights.dim() == 2 and weights.shape[0] == m_total and weights.shape[1] == 1 and d != 1:
        return 0
    if weights.dim() == 2 and weights.shape == (m_total, d):
        return 1
    raise ValueError(f"ensemble_combine: `weights` must be [{m_total}] / [{m_total}, 1] (one per matrix) or [{m_total}, {d}] (one per matrix "
                     f"and column), not {tuple(weights.shape)}")


def _ensemble_outs(out, n_groups, m, d, device):
    """(the n_groups [m, d] outputs, pad_cols): our own padded buffers, or the caller's -- a list, or one [m, n_groups * d] slab"""
    if out is None:
        made = [_alloc_out(m, d, device) for _ in range(n_groups)]
        return [o for o, _ in made], made[0][1]
    if torch.is_tensor(out):
        _check_mat(out, "out")
        if out.shape != (m, n_groups * d) or out.device != device:
            raise ValueError("ensemble_combine: a slab `out` must be [len(idx), n_groups * d] on the matrices' device")
        return [out[:, g * d:(g + 1) * d] for g in range(n_groups)], 0
    outs = list(out)
    if len(outs) != n_groups:
        raise ValueError("ensemble_combine: `out` must hold one matrix per group")
    for g, o in enumerate(outs):
        _check_mat(o, f"out[{g}]")
        if o.shape != (m, d) or o.device != device:
            raise ValueError("ensemble_combine: every `out` matrix must be [len(idx), d] on the matrices' device")
    return outs, 0


def _ensemble_forward(flat, n_groups, gs, w, cs, idx, divisor, outs, pad):
    """the launches of sgl_ensemble_combine_f32: one, or one per run of whole groups when there are more matrices than a call takes"""
    n_rows, d = flat[0].shape
    device = flat[0].device
    m = n_rows if idx is None else int(idx.numel())
    if m == 0 or d == 0:
        return outs
    w = w.detach().to(device=device, dtype=torch.float32)
    if cs:                                   # rows of 16-byte vectors: the kernel then loads a member's weights as it loads its columns
        w = F.pad(w, (0, round_up(d, 4) - d)) if d % 4 else w.contiguous()
    else:
        w = w.reshape(-1, 1).contiguous()
    ldw = w.stride(0)

    def one(lo, cnt):
        ptrs, lds = _lib.hop_arrays(flat[lo * gs:(lo + cnt) * gs])
        optrs, olds = _lib.hop_arrays(outs[lo:lo + cnt])
        return _call(device, "sgl_ensemble_combine_f32", cnt, gs, ptrs, lds, n_rows, _opt_ptr(idx), m, c_void_p(w.data_ptr() + 4 * ldw * lo * gs),
                     ldw, cs, float(divisor), optrs, olds, pad, d, raw=True)

    _split_calls("sgl_ensemble_combine_f32", n_groups, one)
    _wrote(*outs)
    return outs


def _ensemble_backward(flat, n_groups, gs, cs, idx, divisor, gouts):
    """dW [M, d] (cs = 1) or [M] (cs = 0) of sgl_ensemble_combine_bwd_f32, split like the forward"""
    n_rows, d = flat[0].shape
    device = flat[0].device
    m = n_rows if idx is None else int(idx.numel())
    dw = torch.zeros((n_groups * gs, d) if cs else (n_groups * gs,), dtype=torch.float32, device=device)
    if m == 0 or d == 0:
        return dw
    gs_rows = [_grad_rows(g, m, d) for g in gouts]
    lddw = d if cs else 1

    def one(lo, cnt):
        size = int(_call(None, "sgl_ensemble_combine_bwd_scratch", cnt, gs, m, d, cs, raw=True))
        scratch = torch.empty(size, dtype=torch.float32, device=device)
        ptrs, lds = _lib.hop_arrays(flat[lo * gs:(lo + cnt) * gs])
        gptrs, glds = _lib.hop_arrays(gs_rows[lo:lo + cnt])
        return _call(device, "sgl_ensemble_combine_bwd_f32", cnt, gs, ptrs, lds, n_rows, _opt_ptr(idx), m, gptrs, glds, cs, float(divisor),
                     c_void_p(dw.data_ptr() + 4 * lddw * lo * gs), lddw, ptr(scratch), d, raw=True)

    _split_calls("sgl_ensemble_combine_bwd_f32", n_groups, one)
    return dw


class _EnsembleCombine(torch.autograd.Function):
    """out_g = sum_s X_{g,s}[idx] * W[g,s] / divisor with the weight gradient of sgl_ensemble_combine_bwd_f32; the matrices carry none"""

    @staticmethod
    def forward(ctx, w, spec, *flat):
        n_groups, gs, cs, idx, divisor, outs, pad = spec
        ctx.spec = (n_groups, gs, cs, idx, divisor)
        ctx.w_shape = w.shape
        ctx.save_for_backward(*flat)
        return tuple(_ensemble_forward(list(flat), n_groups, gs, w, cs, idx, divisor, outs, pad))

    @staticmethod
    def backward(ctx, *gouts):
        n_groups, gs, cs, idx, divisor = ctx.spec
        flat = list(ctx.saved_tensors)
        dw = _ensemble_backward(flat, n_groups, gs, cs, idx, divisor, gouts) if ctx.needs_input_grad[0] else None
        return (None if dw is None else dw.reshape(ctx.w_shape), None, *([None] * len(flat)))


def ensemble_combine(groups, weights, idx=None, divisor=1.0, out=None):
    """[ sum_s groups[g][s][idx] * weights[g * S + s] / divisor  for g ] in one launch (sgl_ensemble_combine_f32): the aggregators of
    the heterogeneous models (the reference's *OneDimConvolution, models/simple_models.py:5-84) without the gathered copies, the
    stack and the product tensor.  groups: n_groups lists of S float32 CUDA matrices [n_rows, d] (row views of padded hop buffers are
    read in place); weights: member-major, [M, d] (one weight per matrix and column) or [M] / [M, 1] (one per matrix), M = n_groups *
    S; idx: row indices of any kind (None: all rows; a DEVICE index outside the matrices gives a NaN row, host indices raise
    IndexError); divisor: a true division of every sum (1: none).  out: None, a list of n_groups [len(idx), d] matrices, or one
    [len(idx), n_groups * d] slab.  Returns the list of the n_groups results.  Where `weights` requires a gradient it gets one
    (sgl_ensemble_combine_bwd_f32: a fixed two-level reduction, the same bits in every run); the matrices never do.  More matrices
    than one call takes are split by group."""
    flat, n_groups, gs = _ensemble_members(groups)
    n_rows, d = flat[0].shape
    device = flat[0].device
    cs = _ensemble_weight_mode(weights, n_groups * gs, d)
    if idx is not None:
        idx = _device_index(idx, n_rows, device)
    m = n_rows if idx is None else int(idx.numel())
    outs, pad = _ensemble_outs(out, n_groups, m, d, device)
    if weights.requires_grad and torch.is_grad_enabled():
        return list(_EnsembleCombine.apply(weights, (n_groups, gs, cs, idx, divisor, outs, pad), *flat))
    return _ensemble_forward(flat, n_groups, gs, weights, cs, idx, divisor, outs, pad)

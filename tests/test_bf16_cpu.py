"""CPU-side checks of the bfloat16 hop storage: exported symbols, header / binding agreement, the row pitch of 2-byte rows, and the
error contract of the new entry points without a GPU (non-zero code + message, never an abort)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from sgl_amd import _lib
from sgl_amd import device as dev

NEW = ["sgl_spmm_bf16", "sgl_spmm_chain_bf16", "sgl_spmm_acc_bf16", "sgl_gather_rows_bf16_f32", "sgl_gather_hops_bf16_f32"]


def test_library_exports_the_bf16_symbols():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(handle, name), f"{name} is not exported by libsgl_hip.so"
        assert name in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 101


def test_header_and_binding_argument_counts_agree():
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/sgl_hip.h"
        params = [p for p in m.group(1).split(",") if p.strip()]
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), (name, len(argtypes), params)
        # bf16 matrices travel as uint16_t pointers, leading dimensions as int64_t (elements)
        assert "uint16_t" in m.group(1)


def test_row_pitch_default_is_unchanged_and_2_byte_rows_use_whole_vectors():
    assert [dev.row_pitch(d) for d in (12, 100, 147, 500)] == [16, 100, 160, 512]
    assert [dev.row_pitch(d, elem_size=4) for d in (12, 100, 147, 500)] == [16, 100, 160, 512]
    assert dev.expected_lines(100, 100) == 4.0 and dev.expected_lines(160, 147) == 5.0
    for d in list(range(1, 300)) + [500, 512, 520, 1000, 1433]:
        ld = dev.row_pitch(d, elem_size=2)
        ld8 = dev.round_up(d, 8)
        assert ld % 8 == 0 and ld >= d
        assert dev.expected_lines(ld, d, 2) <= dev.expected_lines(ld8, d, 2)
        assert ld <= 1.34 * ld8                                       # the growth cap of the fp32 rule
    assert dev.expected_lines(128, 100, 2) == 2.0 and dev.expected_lines(104, 100, 2) == 2.5
    assert dev.row_pitch(100, elem_size=2) in (104, 128)
    with pytest.raises(ValueError):
        dev.row_pitch(100, elem_size=3)


def test_alloc_rows_dtype_argument_on_cpu():
    t = dev.alloc_rows(5, 100, "cpu")
    assert t.dtype == torch.float32 and t.shape == (5, 100) and t.stride(0) == 100
    b = dev.alloc_rows(5, 100, "cpu", dtype=torch.bfloat16)
    ld = dev.row_pitch(100, elem_size=2)
    assert b.dtype == torch.bfloat16 and b.shape == (5, 100) and b.stride() == (ld, 1)
    parent = dev.padded_parent(b)
    assert parent.shape == (5, ld) and not parent[:, 100:].float().abs().sum().item()
    assert dev.hop_torch_dtype("bfloat16") is torch.bfloat16 and dev.hop_torch_dtype("float32") is torch.float32
    with pytest.raises(ValueError):
        dev.hop_torch_dtype("float16")


def test_config_and_operator_options():
    from sgl_amd import config
    from sgl_amd.operators.graph_op import LaplacianGraphOp, PprGraphOp
    assert config.hop_dtype == os.environ.get("SGL_AMD_HOP_DTYPE", "float32")
    assert "hop_dtype" in config.__doc__ and "SGL_AMD_HOP_DTYPE" in config.__doc__
    for cls in (LaplacianGraphOp, PprGraphOp):
        assert cls(2, hop_dtype="bfloat16")._bf16_hops() is True
        assert cls(2, hop_dtype="float32")._bf16_hops() is False
        for other in ("host_output", "slab_hops"):
            with pytest.raises(ValueError, match=other):
                cls(2, hop_dtype="bfloat16", **{other: True})._bf16_hops()
        with pytest.raises(ValueError):
            cls(2, hop_dtype="half")._bf16_hops()


def _fails_with_message(rc):
    assert rc != 0
    assert len(_lib.last_error()) > 0


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    null = None
    buf = (ctypes.c_uint16 * 64)()
    out = (ctypes.c_float * 64)()
    idx = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    p, o, i = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p), ctypes.cast(idx, ctypes.c_void_p)
    # NULL handle
    _fails_with_message(lib.sgl_spmm_bf16(null, p, 8, p, 8, 8, null))
    assert "sgl_spmm_bf16" in _lib.last_error()
    _fails_with_message(lib.sgl_spmm_chain_bf16(null, 1, p, 8, null, null, 8, null))
    _fails_with_message(lib.sgl_spmm_acc_bf16(null, p, 8, p, 8, 8, o, 8, 1.0, 0, 1.0, null))
    # accumulator arguments are checked before anything else
    _fails_with_message(lib.sgl_spmm_acc_bf16(null, p, 8, p, 8, 8, null, 8, 1.0, 0, 1.0, null))
    _fails_with_message(lib.sgl_spmm_acc_bf16(null, p, 8, p, 8, 8, o, 8, 1.0, 9, 1.0, null))
    _fails_with_message(lib.sgl_spmm_acc_bf16(null, p, 8, p, 8, 8, o, 8, 1.0, 0, 0.0, null))
    # gathers: NULL matrices, pitches smaller than the row, negative sizes, NULL indices, too many hops
    _fails_with_message(lib.sgl_gather_rows_bf16_f32(null, 8, 4, i, 4, o, 8, 8, 0, null))
    _fails_with_message(lib.sgl_gather_rows_bf16_f32(p, 8, 4, i, 4, null, 8, 8, 0, null))
    _fails_with_message(lib.sgl_gather_rows_bf16_f32(p, 4, 4, i, 4, o, 8, 8, 0, null))
    _fails_with_message(lib.sgl_gather_rows_bf16_f32(p, 8, 4, i, 4, o, 8, 8, 4, null))
    _fails_with_message(lib.sgl_gather_rows_bf16_f32(p, 8, 4, i, -1, o, 8, 8, 0, null))
    _fails_with_message(lib.sgl_gather_rows_bf16_f32(p, 8, 4, null, 4, o, 8, 8, 0, null))
    _fails_with_message(lib.sgl_gather_hops_bf16_f32(0, null, null, 4, i, 4, null, null, 8, 0, null))
    _fails_with_message(lib.sgl_gather_hops_bf16_f32(2, null, null, 4, i, 4, null, null, 8, 0, null))
    ptrs = (ctypes.c_void_p * 17)(*[p.value] * 17)
    outs = (ctypes.c_void_p * 17)(*[o.value] * 17)
    lds = (ctypes.c_int64 * 17)(*[8] * 17)
    rc = lib.sgl_gather_hops_bf16_f32(17, ptrs, lds, 4, i, 4, outs, lds, 8, 0, null)
    _fails_with_message(rc)
    assert rc == 1003                                                  # SGL_ERR_UNSUPPORTED: gather hop by hop

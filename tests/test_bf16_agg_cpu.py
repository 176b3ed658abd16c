"""CPU-side checks of the aggregators that read bfloat16 hop matrices in place (csrc/sgl_aggregate_bf16.hip): exported symbols,
header / binding agreement, and the error contract of the four entries without a GPU -- a non-zero code and a message that names
the entry, never an abort, nothing launched."""
import ctypes
import os
import re

from conftest import ROOT

from sgl_amd import _lib

NEW = ["sgl_hop_reduce_bf16_f32", "sgl_hop_concat_bf16", "sgl_hop_concat_bf16_f32", "sgl_nafs_bf16_f32"]
H_MAX = _lib.SGL_MAX_HOPS


def test_library_exports_the_symbols():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(handle, name), f"{name} is not exported by libsgl_hip.so"
        assert name in _lib.PROTOTYPES
    assert _lib.lib().sgl_version() >= 102


def test_header_and_binding_argument_counts_agree():
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/sgl_hip.h"
        params = [p for p in m.group(1).split(",") if p.strip()]
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), (name, len(argtypes), params)
        assert "uint16_t" in m.group(1) and "pad_cols" in m.group(1)


class Args:
    """a valid call of every entry on HOST memory that is never touched (n = 0 returns before any launch; every bad call is refused
    before): four hops of [n, 8] on a pitch of 8, an output pitch of 40 (room for the concatenation and 8 pad columns)"""

    def __init__(self):
        self.buf = (ctypes.c_uint16 * 256)()
        self.out = (ctypes.c_float * 256)()
        self.w = (ctypes.c_float * 64)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.o = ctypes.cast(self.out, ctypes.c_void_p)
        self.wp = ctypes.cast(self.w, ctypes.c_void_p)
        self.kw = dict(op=_lib.SGL_REDUCE_SUM, n_hops=4, d=8, ldx=8, ldo=40, pad=0, n=0, null_hops=False, null_hop=False)

    def hop_arrays(self, n_hops, ldx, null_hop):
        k = max(n_hops, 1)
        ptrs = (ctypes.c_void_p * k)(*[self.p.value] * k)
        if null_hop:
            ptrs[k - 1] = None
        return ptrs, (ctypes.c_int64 * k)(*[ldx] * k)

    def call(self, name, **change):
        a = dict(self.kw, **change)
        ptrs, lds = (None, None) if a["null_hops"] else self.hop_arrays(a["n_hops"], a["ldx"], a["null_hop"])
        lib = _lib.lib()
        if name == "sgl_hop_reduce_bf16_f32":
            return lib.sgl_hop_reduce_bf16_f32(a["op"], a["n_hops"], ptrs, lds, self.wp, self.o, a["ldo"], a["pad"], a["n"], a["d"], None)
        if name == "sgl_nafs_bf16_f32":
            return lib.sgl_nafs_bf16_f32(a["n_hops"], ptrs, lds, self.o, a["ldo"], a["pad"], self.wp, 64, a["n"], a["d"], None)
        return getattr(lib, name)(a["n_hops"], ptrs, lds, self.o, a["ldo"], a["pad"], a["n"], a["d"], None)


def refused(args, name, **change):
    rc = args.call(name, **change)
    msg = _lib.last_error()
    assert rc != 0, (name, change)
    assert msg and name in msg, (name, change, msg)
    return rc


def test_entries_reject_bad_arguments_without_a_gpu():
    a = Args()
    for name in NEW:
        assert a.call(name) == 0, (name, _lib.last_error())                  # n = 0: nothing to do, no device needed
        assert a.call(name, pad=8) == 0, (name, _lib.last_error())
        refused(a, name, null_hops=True)
        refused(a, name, null_hop=True)
        refused(a, name, n_hops=0)
        refused(a, name, n_hops=H_MAX + 1)
        refused(a, name, ldx=7)                                               # ldx < d
        refused(a, name, pad=33)                                              # 8 + 33 > 40, 4 * 8 + 33 > 40
        refused(a, name, pad=-1)
        refused(a, name, ldo=7)
        refused(a, name, d=0)
        refused(a, name, d=-3)
        refused(a, name, n=-1)
        # bad arguments are refused whatever n is
        refused(a, name, n=5, n_hops=0)
        refused(a, name, n=5, ldx=7)
    for op in (-1, 5):
        refused(a, "sgl_hop_reduce_bf16_f32", op=op)
        refused(a, "sgl_hop_reduce_bf16_f32", op=op, n=5)


def test_nafs_refuses_the_shapes_it_does_not_take_with_unsupported():
    """more than 16 hops, d > 512, rows that are not 8-byte aligned / pitches that are no multiple of 4: SGL_ERR_UNSUPPORTED and a
    message that says what to do instead (widen), before anything is launched"""
    a = Args()
    for change in (dict(n_hops=17), dict(n_hops=H_MAX), dict(d=513, ldx=520, ldo=520), dict(d=6, ldx=6, ldo=8), dict(d=8, ldx=8, ldo=10)):
        rc = refused(a, "sgl_nafs_bf16_f32", n=3, **change)
        assert rc == _lib.SGL_ERR_UNSUPPORTED == 1003, (change, rc)
        assert "widen" in _lib.last_error(), _lib.last_error()
        assert a.call("sgl_nafs_bf16_f32", n=0, **change) == 0                # a valid call all the same: no rows, nothing to do

"""CPU-side checks of the sparse x sparse product (csrc/sgl_spgemm.hip, include/sgl_spgemm.h, device.csr_matmul): the exported symbols,
the host rule of the row classes and the window against a restatement, and the refusals that need no GPU."""
import ctypes

import pytest
import torch

from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.io import DeviceAdjacency

CAPS, WINDOWS = (32, 128, 512), (1024, 32768, 524288)


@pytest.mark.parametrize("name", ["sgl_csr_matmul_rule", "sgl_csr_matmul_rowptr", "sgl_csr_matmul_fill"])
def test_library_exports_the_symbols(name):
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib.SPGEMM_PROTOTYPES
    assert (_lib.SGL_SPGEMM_NARROW_CAPS, _lib.SGL_SPGEMM_WINDOWS) == (dev.CSR_MATMUL_NARROW_CAPS, dev.CSR_MATMUL_WINDOWS) == (CAPS, WINDOWS)


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 1500, 32768, 32769, 524288, 524289, (1 << 31) - 1])
def test_the_rule_against_a_restatement(n):
    """auto: the largest cap, the smallest window that covers n columns or else the largest; a compiled value is taken as it is"""
    rule = (ctypes.c_int * 2)()
    auto_window = next((w for w in WINDOWS if w >= n), WINDOWS[-1])
    for cap in (0,) + CAPS:
        for window in (0,) + WINDOWS:
            assert _lib.lib().sgl_csr_matmul_rule(cap, window, n, rule) == 0, _lib.last_error()
            assert tuple(rule) == (cap or CAPS[-1], window or auto_window)
    for cap, window, word in ((31, 0, "narrow_cap"), (64, 0, "narrow_cap"), (-32, 0, "narrow_cap"), (0, 1000, "window_cols"), (0, 2048, "window_cols")):
        assert _lib.lib().sgl_csr_matmul_rule(cap, window, n, rule) != 0 and word in _lib.last_error()


def test_bad_arguments_are_refused_without_a_gpu():
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    total = ctypes.c_int64(-7)
    good = dict(a_rowptr=p, a_col=p, nnz_a=3, b_rowptr=p, b_col=p, nnz_b=3, m=4, k=4, n=4, cap=0, window=0, out=p)

    def rowptr(**change):
        g = dict(good, **change)
        rc = _lib.lib().sgl_csr_matmul_rowptr(g["a_rowptr"], g["a_col"], g["nnz_a"], g["b_rowptr"], g["b_col"], g["nnz_b"], g["m"], g["k"], g["n"],
                                              g["cap"], g["window"], g["out"], ctypes.byref(total), None)
        assert rc != 0 and "sgl_csr_matmul_rowptr" in _lib.last_error(), change

    for key in ("m", "k", "n", "nnz_a", "nnz_b"):
        rowptr(**{key: -1})
    for key in ("m", "k", "n"):
        rowptr(**{key: 1 << 31})
    for key in ("a_rowptr", "a_col", "b_rowptr", "b_col", "out"):
        rowptr(**{key: None})
    rowptr(a_rowptr=ctypes.c_void_p(p.value + 4))
    rowptr(b_col=ctypes.c_void_p(p.value + 2))
    rowptr(cap=64)
    rowptr(window=4096)
    assert total.value == -7                                                  # never written by a refused call
    fill = lambda mode, a_val: _lib.lib().sgl_csr_matmul_fill(p, p, a_val, 3, p, p, p, 3, 4, 4, 4, mode, 0, 0, p, p, p, None)    # noqa: E731
    assert fill(2, p) != 0 and "mode" in _lib.last_error()
    assert fill(0, None) != 0 and "a_val" in _lib.last_error()                # the values are read under SUM ...
    assert _lib.lib().sgl_csr_matmul_fill(p, p, None, 0, p, p, None, 3, 4, 4, 4, 1, 0, 0, p, p, p, None) == 0      # ... and nothing is launched for an empty side


def test_python_layer_refuses_before_any_launch():
    def host(m, n, nnz=0):
        return DeviceAdjacency(torch.zeros(m + 1, dtype=torch.int64), torch.zeros(nnz, dtype=torch.int32), torch.zeros(nnz, dtype=torch.float32), (m, n))

    with pytest.raises(TypeError, match="csr_matmul"):                        # CPU tensors
        dev.csr_matmul(host(3, 4), host(4, 5))
    assert "csr_matmul" in dev.__all__ and dev.CSR_MATMUL_VALUES == {"sum": 0, "ones": 1}

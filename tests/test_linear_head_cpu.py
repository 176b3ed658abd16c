"""CPU-side checks of the fused linear head (csrc/sgl_linear_head.hip, include/sgl_linear_head.h): the exported symbols, the two host
rules against their definition in the header, and the refusals that need no GPU."""
import ctypes

import pytest
import torch

from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.models.homo import GAMLP
from sgl_amd.tricks import classification as cl

TILES = (1, 2, 3, 4, 6, 8)


def test_library_exports_the_symbols():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(handle, name) for name in _lib.LINEAR_HEAD_PROTOTYPES) and len(_lib.LINEAR_HEAD_PROTOTYPES) == 5
    assert _lib.SGL_LINEAR_HEAD_MAX_C == dev.LINEAR_HEAD_MAX_C == 32 * TILES[-1]
    assert "linear_cross_entropy" in cl.__all__


@pytest.mark.parametrize("c", (1, 3, 33, 47, 65, 172, 256))
def test_the_rules_against_the_header(c):
    rule, out = (ctypes.c_int * 4)(), (ctypes.c_int64 * 5)()
    for d in (1, 7, 100, 130, 600):
        nt = next(t for t in TILES if 32 * t >= c)
        dp, budget = -(-d // 8) * 8, 16384 - 32 * nt
        w = dp if c * (dp + 4) <= budget else (budget // c - 4) // 8 * 8
        assert _lib.lib().sgl_linear_class_rule(d, c, rule) == 0, _lib.last_error()
        assert tuple(rule) == (nt, 2 if nt <= 4 else 1, w, w + 4) and w >= 8 and (c * (w + 4) + 32 * nt) * 4 <= 65536
        ct = 1 if c <= 32 else 2 if c <= 64 else 4 if c <= 128 else 8
        slabs = -(-(-(-(d + 1) // 32)) // (8 // ct))
        try:
            for n, forced in ((0, 0), (1, 0), (1031, 0), (2449029, 0), (1031, 3), (1031, 5000)):
                _lib.set_tuning("loss_blocks", forced)
                want = min(forced or max(n // -(-40 * c * (d + 1) // d), 1), 2048, n)
                rows = -(-n // want) if n else 0
                assert _lib.lib().sgl_linear_wgrad_rule(n, d, c, out) == 0, _lib.last_error()
                assert tuple(out) == (-(-n // rows) if n else 0, rows, ct, 8 // ct, slabs)
                assert _lib.lib().sgl_linear_wgrad_scratch(n, d, c) == out[0] * slabs * 32768
        finally:
            _lib.set_tuning("loss_blocks", 0)
    assert _lib.lib().sgl_linear_class_rule(100, 257, rule) == 1003 and "256" in _lib.last_error()
    assert _lib.lib().sgl_linear_wgrad_rule(10, 100, 257, out) == 1003 and _lib.lib().sgl_linear_wgrad_scratch(10, 100, 257) == -1


def test_refusals_before_any_launch():
    p = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    f = _lib.lib().sgl_linear_class_f32
    assert f(p, 8, 0, 8, p, 8, 2, p, p, 1.0, p, p, p, 2, p, 2, None) == 0, _lib.last_error()      # n = 0: nothing to do
    for args in ((p, 7, 0, 8, p, 8, 2, p, p, 1.0, p, p, p, 2, p, 2), (p, 8, 5, 8, p, 8, 2, p, p, 1.0, None, None, None, 0, None, 0),
                 (p, 8, 5, 8, p, 8, 2, p, None, 1.0, p, p, None, 0, None, 0), (p, 8, 0, 8, p, 8, 2, p, p, 1.0, p, p, p, 1, p, 2),
                 (p, 8, 0, 8, p, 8, 257, p, p, 1.0, p, p, p, 257, p, 257)):
        assert f(*args, None) != 0 and "sgl_linear_class_f32" in _lib.last_error(), args
    x = torch.zeros((8, 16))
    with pytest.raises(TypeError):                                      # CPU tensors
        dev.linear_class_loss(x, torch.zeros((3, 16)), None, None, 1.0, pred=True)
    with pytest.raises(ValueError, match="LogisticRegression"):
        cl.evaluate(GAMLP(2, 16, 3, 8, 2), range(4), range(4), torch.zeros(8, dtype=torch.int64), "cpu", fused_head=True)

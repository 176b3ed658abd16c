"""CPU-side checks of the one-pass per-cluster sums (csrc/sgl_cluster_sums.hip, include/sgl_cluster_sums.h, device.cluster_sums): the
exported symbols, the host rule's arithmetic and the refusals that need no GPU."""
import ctypes
import os

import pytest
import torch

from sgl_amd import _lib
from sgl_amd import device as dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 65536                                                          # bytes of LDS: the header's budget
SHAPES = ((2449029, 100, 47), (2449029, 128, 47), (2449029, 600, 47), (1031, 100, 47), (1031, 1, 1), (1031, 7, 2), (1031, 600, 64),
          (1031, 2500, 130), (1, 3, 7), (65, 1030, 1024), (5000000, 33, 1), (300000, 257, 1000))


def rule(n, d, k, vec4=1):
    out = (ctypes.c_int64 * 5)()
    assert _lib.lib().sgl_cluster_sums_rule(n, d, k, vec4, out) == 0, _lib.last_error()
    return tuple(out)


def test_library_exports_the_header_and_nothing_reaches_sgl_hip_h():
    header = open(os.path.join(ROOT, "include", "sgl_cluster_sums.h")).read()
    for name in _lib.CLUSTER_SUMS_PROTOTYPES:
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name + "(" in header
        assert name not in open(os.path.join(ROOT, "include", "sgl_hip.h")).read() and name not in _lib.PROTOTYPES
    assert f"#define SGL_CLUSTER_SUMS_MAX_K {_lib.SGL_CLUSTER_SUMS_MAX_K}\n" in header and dev.CLUSTER_SUMS_MAX_K == _lib.SGL_CLUSTER_SUMS_MAX_K >= 1024


@pytest.mark.parametrize("n,d,k", SHAPES)
def test_the_rule_arithmetic(n, d, k):
    blocks, rows, slab, slabs, lds = rule(n, d, k)
    dp = -(-d // 4) * 4
    assert rule(n, d, k, 0) == (blocks, rows, slab, slabs, lds)
    assert blocks * rows >= n > (blocks - 1) * rows and 1 <= blocks <= 2048
    assert slab % 4 == 0 and slabs * slab >= dp > (slabs - 1) * slab and lds == (k * slab + k) * 4 <= BUDGET
    assert slabs == 1 or (k * (dp + 1)) * 4 > BUDGET                    # the whole row whenever it fits
    assert blocks == 1 or 2 * k * dp * blocks <= 0.05 * n * d + 2 * k * dp   # the tables' traffic: 5 % of X (B is rounded from n / R)
    assert _lib.lib().sgl_cluster_sums_scratch(n, d, k) == blocks * slabs * k * slab * 4 + blocks * k * 4
    try:
        for forced in (1, 3, 4096):
            _lib.set_tuning("loss_blocks", forced)
            b, r = rule(n, d, k)[:2]
            assert b * r >= n > (b - 1) * r and b <= min(forced, n, 2048) and (b == forced or n % forced or forced > min(n, 2048))
            assert _lib.lib().sgl_cluster_sums_scratch(n, d, k) == b * slabs * k * slab * 4 + b * k * 4
    finally:
        _lib.set_tuning("loss_blocks", 0)


def test_refusals_without_a_gpu():
    assert rule(2449029, 100, 47) == (1302, 1881, 100, 1, 47 * 101 * 4) and rule(2449029, 600, 47)[2:4] == (300, 2)
    for n, d in ((0, 100), (1031, 0), (0, 0)):                          # no partial kernel, no scratch
        assert rule(n, d, 47)[:2] == (0, 0) and _lib.lib().sgl_cluster_sums_scratch(n, d, 47) == 0
    out = (ctypes.c_int64 * 5)()
    assert _lib.lib().sgl_cluster_sums_rule(100, 8, 1025, 1, out) == _lib.SGL_ERR_UNSUPPORTED and "1024" in _lib.last_error()
    assert _lib.lib().sgl_cluster_sums_scratch(100, 8, 1025) == -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = _lib.lib().sgl_cluster_sums_f32
    assert f(p, 8, 0, 8, p, 0, p, 8, p, p, None) == 0                   # k = 0: nothing to do, no device needed
    for args in ((p, 8, 5, 8, p, 1025, p, 8, p, p), (p, 7, 5, 8, p, 2, p, 8, p, p), (p, 8, 5, 8, p, 2, p, 7, p, p), (p, 8, -1, 8, p, 2, p, 8, p, p),
                 (None, 8, 5, 8, p, 2, p, 8, p, p), (p, 8, 5, 8, None, 2, p, 8, p, p), (p, 8, 5, 8, p, 2, p, 8, p, None),
                 (p, 8, 5, 8, p, 2, p, 8, p, ctypes.c_void_p(p.value + 4))):
        assert f(*args, None) != 0 and "sgl_cluster_sums_f32" in _lib.last_error(), args
    x = torch.zeros((8, 16))
    with pytest.raises(TypeError):                                      # CPU tensors
        dev.cluster_sums(x, torch.zeros(8, dtype=torch.int64), 2)

"""CPU-side checks of the greedy k-means++ seeding (csrc/sgl_kmeans_seed.hip, include/sgl_kmeans_seed.h, device.kmeans_seed): the exported
symbols, the host rule's arithmetic, the refusals that need no GPU, and the margin the inputs of the GPU float-row tests must leave."""
import ctypes
import os

import numpy as np
import pytest
import torch

from kmeans_common import blob_set, distances64
from kmeans_seed_common import FLOAT_CASES, MARGIN, draws_table, seed_reference
from sgl_amd import _lib
from sgl_amd import device as dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 65536                                                          # bytes of LDS: the header's budget
SHAPES = ((2449029, 100), (2449029, 600), (1031, 1), (1031, 3), (1031, 2048), (1031, 2051), (255, 131), (256, 4), (257, 100), (1, 7),
          (5000000, 33), (5000, 20000))


def rule(n, d, trials):
    out = (ctypes.c_int64 * 5)()
    assert _lib.lib().sgl_kmeans_seed_rule(n, d, trials, out) == 0, _lib.last_error()
    return tuple(out)


def test_library_exports_the_header_and_nothing_reaches_sgl_hip_h():
    header = open(os.path.join(ROOT, "include", "sgl_kmeans_seed.h")).read()
    for name in _lib.KMEANS_SEED_PROTOTYPES:
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name + "(" in header
        assert name not in open(os.path.join(ROOT, "include", "sgl_hip.h")).read() and name not in _lib.PROTOTYPES
    assert f"#define SGL_KMEANS_SEED_MAX_TRIALS {_lib.SGL_KMEANS_SEED_MAX_TRIALS} " in header
    assert dev.KMEANS_SEED_MAX_TRIALS == _lib.SGL_KMEANS_SEED_MAX_TRIALS == 8 == 2 + int(np.log(1096)) < 2 + int(np.log(1097))


@pytest.mark.parametrize("trials", (1, 2, 5, 8))
@pytest.mark.parametrize("n,d", SHAPES)
def test_the_rule_arithmetic(n, d, trials):
    blocks, rows, chunk, chunks, lds = rule(n, d, trials)
    dp = -(-d // 4) * 4
    assert blocks * rows >= n > (blocks - 1) * rows and 1 <= blocks <= 2048
    assert rows == max(256, -(-n // 2048)) == rule(n, 1, 1)[1]          # a function of n alone
    assert chunks * chunk >= dp > (chunks - 1) * chunk and lds == max(4 * trials * chunk, 2048 * trials) <= BUDGET
    assert (chunk == dp) if trials * dp * 4 <= BUDGET else (chunk % 256 == 0 and (chunk + 256) * trials * 4 > BUDGET)
    assert chunks == 1 or d > 2048                                      # the register layouts always hold the candidates whole
    scratch = 2048 * 8 * 8 + 8 * 8 + 16 + 2 * (-(-trials * n * 4 // 16) * 16)
    assert _lib.lib().sgl_kmeans_seed_scratch(n, trials) == scratch
    try:
        for forced in (1, 3, 4096):
            _lib.set_tuning("loss_blocks", forced)
            b, r = rule(n, d, trials)[:2]
            assert b * r >= n > (b - 1) * r and b <= min(forced, n, 2048) and (b == forced or n % forced or forced > min(n, 2048))
            assert rule(n, d, trials)[2:] == (chunk, chunks, lds) and _lib.lib().sgl_kmeans_seed_scratch(n, trials) == scratch
    finally:
        _lib.set_tuning("loss_blocks", 0)


def test_refusals_without_a_gpu():
    assert rule(2449029, 100, 5) == (2048, 1196, 100, 1, 10240) and rule(1031, 2051, 8)[2:4] == (2048, 2)
    out = (ctypes.c_int64 * 5)()
    for trials in (0, 9):
        assert _lib.lib().sgl_kmeans_seed_rule(100, 8, trials, out) == _lib.SGL_ERR_UNSUPPORTED and "[1, 8]" in _lib.last_error()
        assert _lib.lib().sgl_kmeans_seed_scratch(100, trials) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = _lib.lib().sgl_kmeans_seed_f32
    assert f(p, 8, 5, 8, 2, 9, p, p, p, p, p, None) == _lib.SGL_ERR_UNSUPPORTED
    for args in ((p, 8, 5, 8, 0, 2, p, p, p, p, p), (p, 8, 5, 8, 6, 2, p, p, p, p, p), (p, 7, 5, 8, 2, 2, p, p, p, p, p),
                 (None, 8, 5, 8, 2, 2, p, p, p, p, p), (p, 8, 5, 8, 2, 2, None, p, p, p, p), (p, 8, 5, 8, 2, 2, p, p, p, p, None),
                 (p, 8, 5, 8, 2, 2, ctypes.c_void_p(p.value + 4), p, p, p, p)):
        assert f(*args, None) != 0 and "sgl_kmeans_seed_f32" in _lib.last_error(), args
    with pytest.raises(TypeError):                                      # CPU tensors
        dev.kmeans_seed(torch.zeros((8, 16)), 2, torch.zeros((2, 2), dtype=torch.float64), 2)


@pytest.mark.parametrize("blob,trials,seed", FLOAT_CASES)
def test_the_float_inputs_leave_the_margin(blob, trials, seed):
    """with float64 distances rounded to float32 in place of the kernel's: the GPU test asserts the same on the kernel's own"""
    n, d, k, spread = blob
    x = blob_set(n, d, k, spread)[0]
    margin = seed_reference(lambda c: distances64(x, x[c:c + 1])[:, 0].astype(np.float32), n, k, trials, draws_table(k, trials, seed))[3]
    assert margin >= MARGIN, margin

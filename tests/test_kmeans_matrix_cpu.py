"""CPU-side checks of the matrix-core k-means assignment (csrc/sgl_kmeans_mfma.hip, include/sgl_kmeans_mfma.h, device.kmeans_assign
form="matrix"): the exported symbols, the host rule against a restatement, and the refusals that need no GPU."""
import ctypes

import pytest
import torch

from sgl_amd import _lib
from sgl_amd import device as dev

NAME = "sgl_kmeans_assign_matrix_f32"
TILES = (1, 2, 3, 4, 6, 8)


@pytest.mark.parametrize("name", [NAME, "sgl_kmeans_assign_matrix_rule"])
def test_library_exports_the_symbols(name):
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib.KMEANS_MATRIX_PROTOTYPES
    assert _lib.SGL_KMEANS_MATRIX_MAX_K == dev.KMEANS_MATRIX_MAX_K == 32 * TILES[-1]


@pytest.mark.parametrize("vec4", (0, 1))
@pytest.mark.parametrize("k", (1, 32, 33, 64, 65, 128, 129, 256))
def test_the_rule_against_a_restatement(k, vec4):
    """the smallest compiled tile count that covers k; two row tiles up to four centre tiles; all columns (rounded up to 8) while the
    k rows on a pitch of + 4 fit 16384 floats beside the shift and the norms, else the widest multiple of 8 that does"""
    rule = (ctypes.c_int * 4)()
    for d in (1, 8, 9, 100, 147, 600, 640, 5000):
        nt = next(t for t in TILES if 32 * t >= k)
        dp, budget = -(-d // 8) * 8, 16384 - 32 * nt
        w = dp if k * (dp + 4) + dp <= budget else (budget - 4 * k) // (k + 1) // 8 * 8
        assert _lib.lib().sgl_kmeans_assign_matrix_rule(d, k, vec4, rule) == 0, _lib.last_error()
        assert tuple(rule) == (nt, 2 if nt <= 4 else 1, w, w + 4) and w >= 8 and (k * (w + 4) + w + 32 * nt) * 4 <= 65536
    assert _lib.lib().sgl_kmeans_assign_matrix_rule(100, 257, vec4, rule) != 0 and "256" in _lib.last_error()


def test_entry_rejects_bad_arguments_without_a_gpu():
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(x=p, ldx=8, n=0, d=8, c=p, ldc=8, k=2, shift=p, labels=p, dist=p)

    def call(**change):
        g = dict(good, **change)
        return _lib.lib().sgl_kmeans_assign_matrix_f32(g["x"], g["ldx"], g["n"], g["d"], g["c"], g["ldc"], g["k"], g["shift"], g["labels"], g["dist"], None)

    for ok in ({}, dict(d=0), dict(dist=None), dict(shift=None), dict(k=0), dict(x=None, labels=None, dist=None), dict(k=256)):
        assert call(**ok) == 0, (ok, _lib.last_error())                 # n = 0: nothing to do, no device needed
    off = lambda by: ctypes.c_void_p(p.value + by)                      # noqa: E731
    bad = [dict(n=n, **c) for n in (0, 5) for c in (dict(d=-1), dict(k=-1), dict(ldx=7), dict(ldc=7), dict(x=off(2)), dict(c=off(2)), dict(shift=off(2)),
                                                    dict(dist=off(2)), dict(labels=off(4)), dict(k=257))]
    for change in bad + [dict(n=5, x=None), dict(n=5, c=None), dict(n=5, labels=None), dict(n=5, k=0), dict(n=-1)]:
        assert call(**change) != 0 and NAME in _lib.last_error(), (change, _lib.last_error())
    assert call(k=257) == 1003 and "256" in _lib.last_error()          # SGL_ERR_UNSUPPORTED, and the limit by name


def test_python_layer_refuses_before_any_launch():
    x, c = torch.zeros((8, 16)), torch.zeros((2, 16))
    with pytest.raises(TypeError):                                      # CPU tensors
        dev.kmeans_assign(x, c, form="matrix")
    with pytest.raises(ValueError, match="shift"):
        dev.kmeans_assign(x, c, shift=torch.zeros(16))
    with pytest.raises(ValueError, match="256"):
        dev.kmeans_assign(x, torch.zeros((257, 16)), form="matrix")
    with pytest.raises(ValueError, match="form"):
        dev.kmeans_assign(x, c, form="expanded")

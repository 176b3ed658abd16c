"""CPU-side checks of the fused linear head on stored rows (include/sgl_linear_rows.h): the exported symbols and the refusals that
need no GPU."""
import ctypes

import pytest
import torch

from sgl_amd import _lib
from sgl_amd import device as dev

P = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
HEAD = (P, 8, 2, P, P, 1.0)                                            # W, ldw, C, bias, labels, w
# x, ldx, n_rows, idx, m, d, then the head and the outputs: C > 256; m != n_rows without an index; a table without rows; no output;
# negative sizes
CLASS_REFUSALS = ((P, 8, 4, P, 4, 8, P, 8, 257, P, P, 1.0, P, P, P, 257, P, 257), (P, 8, 4, None, 5, 8, *HEAD, P, P, P, 2, P, 2),
                  (P, 8, 0, P, 5, 8, *HEAD, P, P, P, 2, P, 2), (P, 8, 4, P, 4, 8, *HEAD, None, None, None, 0, None, 0),
                  (P, 8, 4, P, -1, 8, *HEAD, P, P, P, 2, P, 2), (P, 8, -1, P, 4, 8, *HEAD, P, P, P, 2, P, 2))
# x, ldx, n_rows, idx, m, d, dz, lddz, C, dw, lddw, db, scratch
WGRAD_REFUSALS = ((P, 8, 4, P, 4, 8, P, 257, 257, P, 8, P, P), (P, 8, 4, None, 5, 8, P, 2, 2, P, 8, P, P), (P, 8, 0, P, 5, 8, P, 2, 2, P, 8, P, P),
                  (P, 8, 4, P, -1, 8, P, 2, 2, P, 8, P, P), (P, 8, -1, P, 4, 8, P, 2, 2, P, 8, P, P))


@pytest.mark.parametrize("kind", ("f32", "bf16"))
def test_symbols_and_refusals_before_any_launch(kind):
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(handle, name) for name in _lib.LINEAR_ROWS_PROTOTYPES) and len(_lib.LINEAR_ROWS_PROTOTYPES) == 4
    for name, refusals, nothing in ((f"sgl_linear_class_rows_{kind}", CLASS_REFUSALS, (P, 8, 4, P, 0, 8, *HEAD, P, P, P, 2, P, 2)),
                                    (f"sgl_linear_wgrad_rows_{kind}", WGRAD_REFUSALS, (P, 8, 4, P, 0, 8, P, 2, 0, P, 8, P, P))):
        f = getattr(_lib.lib(), name)
        assert f(*nothing, None) == 0, _lib.last_error()              # m = 0 (the weight gradient: and C = 0): no launch
        for args in refusals:
            assert f(*args, None) != 0 and name in _lib.last_error(), args
        assert f(*refusals[0], None) == 1003                           # SGL_ERR_UNSUPPORTED


@pytest.mark.parametrize("table", (torch.zeros((8, 16)), torch.zeros((8, 16)).half(), torch.zeros(16)), ids=("host", "float16", "vector"))
def test_the_device_functions_refuse_with_value_errors(table):
    with pytest.raises(ValueError, match="linear_class_loss_rows"):
        dev.linear_class_loss_rows(table, None, torch.zeros((3, 16)), None, None, 1.0, pred=True)
    with pytest.raises(ValueError, match="linear_wgrad_rows"):
        dev.linear_wgrad_rows(table, [0, 1], torch.zeros((8, 3)))

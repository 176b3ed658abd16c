"""CPU-side checks of the one-pass linear-head step (include/sgl_linear_step.h): the exported symbols and where they are declared, the
rule's arithmetic on both sides of the tile limit, and the refusals that need no GPU."""
import ctypes
import os
import re

import pytest
import torch

from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.models.homo import GAMLP
from sgl_amd.tricks import classification as cl

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
P = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)


def test_the_symbols_are_exported_and_declared_in_their_own_header():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    text = {name: open(os.path.join(INCLUDE, name)).read() for name in os.listdir(INCLUDE)}
    for name in _lib.LINEAR_STEP_PROTOTYPES:
        assert hasattr(handle, name)
        assert [h for h in sorted(text) if re.search(rf"\b{name}\(", text[h])] == ["sgl_linear_step.h"], name


@pytest.mark.parametrize("d,c", ((100, 47), (127, 64), (128, 64), (222, 32), (223, 32), (255, 32), (256, 32), (63, 128), (64, 128), (31, 129),
                                 (31, 256), (32, 256), (100, 257)))
def test_the_rule_is_the_headers(d, c, n=100000):
    ct = 1 if c <= 32 else 2 if c <= 64 else 4
    tu = (d + 1 + 31) // 32
    out, wgrad = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 5)()
    rc = _lib.lib().sgl_linear_step_rule(n, d, c, out)
    if c > 128 or tu > {1: 7, 2: 4, 4: 2}[ct]:
        assert rc == 1003 and "sgl_linear_step_rule" in _lib.last_error() and _lib.lib().sgl_linear_step_scratch(n, d, c) == -1
        with pytest.raises(ValueError, match="sgl_linear_step_rule"):
            dev.linear_step_rule(n, d, c)
        return
    assert rc == 0 and _lib.lib().sgl_linear_wgrad_rule(n, d, c, wgrad) == 0
    lds = 4 * max(c * (8 * ((d + 7) // 8) + 4) + 32 * ct + 4 * 32 * 36, 8192)
    assert tuple(out) == (wgrad[0], wgrad[1], ct, tu, lds) == dev.linear_step_rule(n, d, c) and lds <= 53760
    assert _lib.lib().sgl_linear_step_scratch(n, d, c) == out[0] * 8192 * 4


# x, ldx, n_rows, idx, m, then d, W, ldw, C, bias, labels, w, row_loss, pred, dW, lddw, db, scratch: NULL dW; a pitch of dW below d;
# C beyond the rule; a shape outside the rule; m != n_rows without an index
REFUSALS = (((P, 8, 4, P, 4), (8, P, 8, 2, P, P, 1.0, P, P, None, 8, P, P), 1001), ((P, 8, 4, P, 4), (8, P, 8, 2, P, P, 1.0, P, P, P, 7, P, P), 1001),
            ((P, 8, 4, P, 4), (8, P, 8, 257, P, P, 1.0, P, P, P, 8, P, P), 1003), ((P, 128, 4, P, 4), (128, P, 128, 64, P, P, 1.0, P, P, P, 128, P, P), 1003),
            ((P, 8, 4, None, 5), (8, P, 8, 2, P, P, 1.0, P, P, P, 8, P, P), 1001))


@pytest.mark.parametrize("kind", ("f32", "rows_f32", "rows_bf16"))
def test_refusals_before_any_launch(kind):
    f = getattr(_lib.lib(), f"sgl_linear_step_{kind}")
    for table, tail, code in REFUSALS[:4 if kind == "f32" else 5]:
        args = (table[0], table[1], table[4]) if kind == "f32" else table
        assert f(*args, *tail, None) == code and f"sgl_linear_step_{kind}" in _lib.last_error(), (table, tail)


def test_value_errors_without_a_gpu():
    w, y = torch.zeros((3, 16)), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match="linear_step"):
        dev.linear_step(torch.zeros((8, 16)), w, None, y, 1.0)
    with pytest.raises(ValueError, match="linear_step_rows"):
        dev.linear_step_rows(torch.zeros((8, 16)), [0, 1], w, None, y[:2], 1.0)
    model = GAMLP(2, 16, 3, 8, 2)
    with pytest.raises(ValueError, match="LogisticRegression"):
        cl.train(model, range(8), y, "cpu", torch.optim.SGD(model.parameters(), lr=0.1), fused_head="one_pass")
    with pytest.raises(ValueError, match="one_pass_in_place"):
        cl.train(model, range(8), y, "cpu", None, fused_head="one_pass_everywhere")

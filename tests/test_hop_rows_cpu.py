"""CPU-side checks of the learnable hop aggregators on stored rows (include/sgl_hop_rows.h): the exported symbols and where they are
declared, the refusals that need no GPU, and that nothing changes while config.aggregate_in_place is off."""
import ctypes
import os
import re

import pytest
import torch

from sgl_amd import _lib, config
from sgl_amd import device as dev
from sgl_amd.models.homo import GAMLP

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
P = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
TABLES = lambda n: (ctypes.c_void_p * n)(*[P.value] * n)   # noqa: E731
LDS = lambda n, ld: (ctypes.c_int64 * n)(*[ld] * n)      # noqa: E731
# what follows the row source (n_hops, tables, pitches, n_rows, idx, m) in each entry, d included
TAILS = {"scores": (P, 8, 0, P, 0, 1, P, 1, P, 8), "wsum": (P, 1, P, 8, 0, 8), "wsum_bwd": (P, 8, P, 1, 8), "colsum": (P, 1, 1, P, 8, P, 8)}


def test_the_symbols_are_exported_and_declared_in_their_own_header():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    text = {name: open(os.path.join(INCLUDE, name)).read() for name in os.listdir(INCLUDE)}
    assert len(_lib.HOP_ROWS_PROTOTYPES) == 9
    for name in _lib.HOP_ROWS_PROTOTYPES:
        assert hasattr(handle, name) and name not in _lib.PROTOTYPES
        assert [h for h in sorted(text) if re.search(rf"\b{name}\(", text[h])] == ["sgl_hop_rows.h"], name


@pytest.mark.parametrize("kind", ("f32", "bf16"))
@pytest.mark.parametrize("entry", sorted(TAILS))
def test_refusals_before_any_launch(entry, kind):
    name, tail = f"sgl_hop_rows_{entry}_{kind}", TAILS[entry]
    f = getattr(_lib.lib(), name)
    wide = tail[:-1] + (513,)
    # NULL tables; more than 16 tables; d > 512; a pitch that is no multiple of 4; m != n_rows without an index
    for source, t, code in (((1, None, LDS(1, 8), 4, P, 4), tail, 1001), ((17, TABLES(17), LDS(17, 8), 4, P, 4), tail, 1003),
                            ((1, TABLES(1), LDS(1, 516), 4, P, 4), wide, 1003), ((1, TABLES(1), LDS(1, 9), 4, P, 4), tail, 1003),
                            ((1, TABLES(1), LDS(1, 8), 4, None, 5), tail, 1001)):
        assert f(*source, *t, None) == code and name in _lib.last_error(), (source, _lib.last_error())
    assert f(1, TABLES(1), LDS(1, 8), 4, P, 0, *tail, None) == 0, _lib.last_error()      # m = 0: nothing is launched


def test_the_device_functions_refuse_with_value_errors():
    host, w = [torch.zeros((8, 16)) for _ in range(2)], torch.zeros((2, 2))
    assert not dev.hop_rows_fusable(host) and not dev.hop_rows_fusable([])
    with pytest.raises(ValueError, match="hop_scores2_rows"):
        dev.hop_scores2_rows(host, [0, 1], torch.zeros(16), None, 0, 0, 2)
    with pytest.raises(ValueError, match="hop_wsum2d_rows"):
        dev.hop_wsum2d_rows(host, [0, 1], w)
    with pytest.raises(ValueError, match="hop_colsum_rows"):
        dev.hop_colsum_rows(host, [0, 1], w)


def test_forward_does_not_ask_for_rows_while_the_option_is_off(monkeypatch):
    assert config.aggregate_in_place is False
    model = GAMLP(2, 16, 3, 8, 2)
    model._processed_feat_list, model._pre_msg_learnable = [torch.randn(8, 16) for _ in range(3)], True
    asked = []
    monkeypatch.setattr(type(model._pre_msg_op), "aggregate_rows", lambda self, feats, idx: asked.append(idx))
    monkeypatch.setattr(type(model._pre_msg_op), "aggregate", lambda self, hops: torch.ones((hops[0].shape[0], 16)))
    want = model.eval()(range(4), "cpu")
    assert not asked and want.shape == (4, 3)
    monkeypatch.setattr(config, "aggregate_in_place", True)              # on: asked first; None -> the gathered route, the same result
    assert torch.equal(model(range(4), "cpu"), want) and asked == [range(4)]
    model(range(4), "meta")                                              # hops that do not live on the step's device: never asked
    assert asked == [range(4)]

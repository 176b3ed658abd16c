"""The row-layout helpers of sgl_amd.device against the expressions they replaced.  Every site that now calls rows_vectored /
pitch_vectored / own_out_pad / leading_dim used to spell its own test of "are these rows 16-byte vectors", its own pad rule or its
own leading dimension; each of those expressions is restated here as it stood and compared with the helper call that took its place,
over CPU tensors cut with as_strided from storages of an exact size (the helpers look at shape, strides, storage offset, element
size, base address and storage size only)."""
import itertools

import torch

from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.device import round_up, row_pitch, rows_vectored

F32, BF16 = torch.float32, torch.bfloat16


def grid(dtypes=(F32, BF16)):
    """(n, d, tensor): n in {1, 2, 3}, d in {1 .. 500}, five pitches, storage offsets of 0 / 1 / 4 elements, the storage ending at the
    last row's round_up(d, 4) or short of it -- clipped to the row's own d columns, the least a view can be cut from"""
    for dtype, n, d in itertools.product(dtypes, (1, 2, 3), (1, 3, 4, 5, 12, 100, 147, 500)):
        for pitch in (d, round_up(d, 4), row_pitch(d), row_pitch(d) + 4, d + 1):
            for off, end in itertools.product((0, 1, 4), (round_up(d, 4), max(d, round_up(d, 4) - 4))):
                store = torch.empty(off + (n - 1) * pitch + end, dtype=dtype)
                yield n, d, torch.as_strided(store, (n, d), (pitch, 1), off)


def room_f32(x, ld, width):
    return x.untyped_storage().nbytes() // 4 - x.storage_offset() >= (x.shape[0] - 1) * ld + width


def test_the_grid_is_what_it_says():
    cases = list(grid())
    assert len(cases) == 2 * 3 * 8 * 5 * 3 * 2
    assert {t.data_ptr() % 16 for _, _, t in cases} >= {0, 2, 4, 8}
    assert any(not room_f32(t, t.stride(0), round_up(d, 4)) for _, d, t in grid((F32,)))


def test_own_pad():
    for n, d, t in grid():
        ld = t.stride(0)
        was = 0 if n <= 1 else (ld - d if (ld > d and (ld * t.element_size()) % 16 == 0 and t.stride(1) == 1 and t.data_ptr() % 16 == 0) else 0)
        assert dev.own_pad(t) == was, (n, d, t.stride(), t.dtype)


def widened_was(feats, out):
    n, d = out.shape
    strides = {t.stride(0) for t in list(feats) + [out]} if n > 1 else set()
    if len(strides) == 1 and next(iter(strides)) % 4 == 0 and next(iter(strides)) > d:
        dp = next(iter(strides))
    else:
        dp = round_up(d, 4)
    if d == dp or n <= 1:
        return feats, out, d
    ok = all(f.stride(0) % 4 == 0 and f.stride(0) >= dp and f.data_ptr() % 16 == 0 for f in list(feats) + [out])
    if not ok:
        return feats, out, d
    wide = [torch.as_strided(f, (n, dp), (f.stride(0), 1), f.storage_offset()) for f in feats]
    return wide, torch.as_strided(out, (n, dp), (out.stride(0), 1), out.storage_offset()), dp


def test_widened():
    def key(form, feats, out):
        try:
            feats, out, d = form(feats, out)
        except RuntimeError:      # neither form asks whether the storage holds the widened view of the last row: torch refuses it
            return "no room"
        return [(tuple(t.shape), t.stride(), t.data_ptr()) for t in list(feats) + [out]], d
    for n, d, t in grid((F32,)):
        for out in (dev.alloc_rows(n, d, "cpu"), t):
            assert key(dev._widened, [t, t], out) == key(widened_was, [t, t], out), (n, d, t.stride())


def test_single_row_sites():
    """hop_colsum, gate_fusable (a single row passes), _wsum2d_backward (it does not arise: n > 1 there)"""
    for n, d, f in grid((F32,)):
        was = f.data_ptr() % 16 == 0 and (n == 1 or f.stride(0) % 4 == 0)                       # hop_colsum (n > 0)
        assert rows_vectored(f, single_row=True) == was
        was = f.data_ptr() % 16 == 0 and (f.shape[0] == 1 or f.stride(0) % 4 == 0)              # gate_fusable
        assert rows_vectored(f, single_row=True) == was
        if n > 1:                                                                               # _wsum2d_backward: copy the gradient?
            assert (not rows_vectored(f)) == (f.stride(0) % 4 != 0 or f.data_ptr() % 16 != 0)
    assert dev.gate_fusable([dev.alloc_rows(3, 5, "cpu")]) is False                             # (is_cuda stays at the site)


def test_column_signature_site():
    for n, d, x in grid((F32,)):
        dw = round_up(d, 4)
        ld = x.stride(0) if n > 1 else dw
        was = not (x.stride(1) != 1 or ld % 4 or ld < dw or x.data_ptr() % 16) and room_f32(x, ld, dw)
        assert (x.stride(1) == 1 and rows_vectored(x, single_row=True, width=dw, room=True)) == was, (n, d, x.stride())
        assert _lib.leading_dim(x, one_row=dw) == ld


def test_gather_sites():
    """_gather_hops_one_launch's test of every source, gather_rows' `fast` and `vec_ok`, and the pad of an own / a caller's output"""
    for n_rows, d, x in grid((F32,)):
        dp = round_up(d, 4)
        src = rows_vectored(x, width=dp, room=True)
        if n_rows >= 2:                                                                         # one launch over all hops
            was = (x.stride(0) % 4 == 0 and x.stride(0) >= dp and x.data_ptr() % 16 == 0
                   and x.untyped_storage().nbytes() // 4 - x.storage_offset() >= (n_rows - 1) * x.stride(0) + dp)
            assert src == was, (n_rows, d, x.stride())
        for m, out in ((1, dev.alloc_rows(1, d, "cpu")), (3, dev.alloc_rows(3, d, "cpu")), (x.shape[0], x)):
            own_out = out is not x
            fast = (n_rows > 1 and m > 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and 0 < row_pitch(d) - d < 32
                    and x.stride(0) >= dp and room_f32(x, x.stride(0), dp))
            ldx, ldo = x.stride(0) if n_rows > 1 else max(x.stride(0), d), out.stride(0) if m > 1 else max(out.stride(0), d)
            vec_ok = (n_rows > 1 and m > 1 and ldx % 4 == 0 and ldx >= dp and ldo % 4 == 0 and ldo >= dp and room_f32(x, ldx, dp)
                      and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0)
            pad_was = ((ldo - d) if (own_out and ldo - d < 32) else (dp - d)) if vec_ok else 0
            vec = m > 1 and src and rows_vectored(out, width=dp)
            assert vec == vec_ok, (n_rows, d, m, x.stride())
            pad = (dev.own_out_pad(out.stride(0), d) if own_out else dp - d) if vec else 0
            assert pad == pad_was
            if own_out:          # what the kernel does not zero of our own output is zeroed before: all of it unless `fast`
                assert (not fast) or pad == out.stride(0) - d


def test_own_out_pad_rule():
    for d in (1, 3, 4, 5, 12, 100, 147, 500):
        for ldo in {round_up(d, 4), row_pitch(d), row_pitch(d) + 4, d + 40}:
            assert dev.own_out_pad(ldo, d) == ((ldo - d) if ldo - d < 32 else (round_up(d, 4) - d))


def test_graph_op_sites():
    """GraphOp._device_features' re-pack test and the `stride(0) % 4` that picks the padded parent"""
    for n, d, cur in grid((F32,)):
        was = (cur.shape[1] > 1 and cur.stride(1) != 1) or cur.data_ptr() % 16 != 0 or \
            (cur.shape[0] > 1 and cur.stride(0) != row_pitch(cur.shape[1]))
        now = (cur.shape[1] > 1 and cur.stride(1) != 1) or not rows_vectored(cur, single_row=True) or \
            (cur.shape[0] > 1 and cur.stride(0) != row_pitch(cur.shape[1]))
        assert now == was
        assert dev.pitch_vectored(cur) == (cur.stride(0) % 4 == 0)


def test_leading_dimensions():
    """device._ld, _lib.hop_arrays and the gradient arrays built by hand: three values for a one-row view, kept as they were"""
    for n, d, t in grid():
        assert _lib.leading_dim(t) == (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1))
        ptrs, lds = _lib.hop_arrays([t, None, t])
        assert list(lds) == [t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)), 0] * 1 + [lds[0]] and lds[2] == lds[0]
        assert [ptrs[0], ptrs[1], ptrs[2]] == [t.data_ptr(), None, t.data_ptr()]
        ptrs, lds = _lib.hop_arrays([None, t], one_row_pitch=False)
        assert list(lds) == [0, t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)] and ptrs[0] is None

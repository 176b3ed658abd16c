"""The layout arithmetic of the far-offset tests (far_common.py) on meta tensors: no memory, no GPU.

What is checked here is what makes test_gpu_far_offsets.py able to fail: every matrix it hands a kernel has rows beyond the tier's
threshold, satisfies the strictest vector rule in use, overlaps no other matrix of the test -- and a row offset that wraps at 32
bits lands on ANOTHER row (hashed inputs differ row by row) or on the NaN fill, never on the row itself."""
import pytest
import torch

from far_common import (ALIGN_BYTES, FILL32, GIB, SLACK, TIERS, ZONE, ZONE_BYTES, FarTable, default_pitch_rows, far_pitch, pick_tier,
                        table_elems)

NS = (2, 333, 515, 1500, 4099)
DTYPES = (torch.float32, torch.bfloat16)
WIDTHS = (104, 147, 11, 4, 512)             # what the GPU tests take: two hop widths, a score matrix, a concat half


def meta_table(tier):
    return FarTable(torch.empty(table_elems(tier), dtype=torch.float32, device="meta"), TIERS[tier][1])


def test_table_sizes_and_tiers():
    assert table_elems("A") == 2 ** 32 + 2 ** 27 and table_elems("B") == 2 ** 31 + 2 ** 27
    assert 17.0e9 < table_elems("A") * 4 < 18.0e9 and 8.6e9 < table_elems("B") * 4 < 9.2e9
    assert TIERS["A"] == (24 * GIB, 2 ** 32) and TIERS["B"] == (12 * GIB, 2 ** 31)
    assert pick_tier(200 * GIB) == "A" and pick_tier(24 * GIB) == "A" and pick_tier(24 * GIB - 1) == "B"
    assert pick_tier(12 * GIB) == "B" and pick_tier(12 * GIB - 1) is None
    for tier in TIERS:                                                    # the table leaves room for the sweep's temporaries
        assert table_elems(tier) * 4 + 2 * GIB < TIERS[tier][0]
    assert FILL32 < 2 ** 31 and (FILL32 >> 16) == (FILL32 & 0xFFFF) == 0x7FC0
    assert (FILL32 >> 23) & 0xFF == 0xFF and FILL32 & 0x7FFFFF             # a float32 NaN
    assert ZONE >= 16 * 512 + 2 * 512 and ZONE_BYTES == 4 * ZONE and SLACK >= ZONE


@pytest.mark.parametrize("n", NS)
def test_far_pitch(n):
    for thr in (2 ** 31, 2 ** 32):
        for m in (4, 8):
            ld = far_pitch(n, thr, m)
            assert ld % m == 0 and (n - 1) * ld > thr
            assert n == 2 or (n - 1) * (ld - m) <= thr                     # the smallest such pitch


@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("n", NS)
def test_views_are_far_aligned_and_disjoint(tier, n):
    table = meta_table(tier)
    thr = table.threshold
    lay = table.layout(n)
    assert (n - 1) * lay.ld > thr and (n - 1) * 2 * lay.ld > thr           # float32 and bfloat16 pitch
    assert (n - 1) * lay.ld + ZONE <= table.flat.numel()
    assert lay.ld >= 2 * ZONE                                              # rows of the table do not run into each other's zones
    views = [lay.take(d, dt) for dt in DTYPES for d in WIDTHS]
    for v in views:
        e = 2 if v.dtype == torch.bfloat16 else 4
        ld = v.t.stride(0) if n > 1 else None
        assert v.t.shape == (n, v.t.shape[1]) and v.t.stride(1) == 1 and v.t.dtype == v.dtype
        assert ld * e == lay.ld * 4 == v.row_bytes
        # the strictest vector rule in use: 16-byte bases; float32 pitches multiples of 4, bfloat16 ones of 8
        assert v.byte_col % ALIGN_BYTES == 0 and ALIGN_BYTES % 16 == 0 and all(b % 16 == 0 for b in v.byte_offsets()[:3] + v.byte_offsets()[-3:])
        assert ld % (4 if e == 4 else 8) == 0
        assert v.byte_col + v.width_bytes <= ZONE_BYTES and v.width_bytes >= v.t.shape[1] * e
        offs = v.elem_offsets()
        assert offs == [v.t.storage_offset() + r * ld for r in range(n)]
        assert offs[-1] > thr
        assert offs[-1] + v.t.shape[1] <= table.flat.numel() * (4 // e)    # the last row lies inside the allocation
        if tier == "A":
            assert v.far_rows(2 ** 32) >= 1
        if tier == "A" or e == 2:
            assert v.far_rows(2 ** 31) >= max(n // 4, 1)
        else:
            assert v.far_rows(2 ** 31) >= 1
    spans = sorted((v.byte_col, v.byte_col + v.width_bytes) for v in views)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))             # column ranges of one test do not overlap
    with pytest.raises(ValueError):                                        # nothing is handed out at or beyond ZONE
        for _ in range(100):
            lay.take(512)
    assert lay.cursor <= ZONE_BYTES


# the layouts test_gpu_far_offsets.py builds: (rows, rows the pitch is computed for, (rows, step) of a strided view or None)
KMEANS_N, KMEANS_K = 1031, 64
KMEANS_STEP = (KMEANS_N - 1) // (KMEANS_K - 1)
GPU_LAYOUTS = [(n, default_pitch_rows(n), None) for n in (1500, 515, 257)] + \
              [(515, default_pitch_rows(515), (11, 514 // 10)), (515, default_pitch_rows(515), (4, 514 // 3)),      # colsum outputs, U
               (KMEANS_N, (KMEANS_K - 1) * KMEANS_STEP + 1, (KMEANS_K, KMEANS_STEP))]                                # k-means centres
ALL_LAYOUTS = [(n, None, None) for n in NS] + GPU_LAYOUTS


@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("n,pitch_rows,strided", ALL_LAYOUTS, ids=lambda v: str(v).replace(" ", ""))
def test_a_wrapped_offset_lands_where_the_values_differ(tier, n, pitch_rows, strided):
    """For every row of every view that starts beyond the threshold -- in the plain layouts and in each layout the GPU tests build,
    strided views included -- the place its offset wraps to when taken modulo 2^32 elements (an unsigned 32-bit element index),
    modulo 2^32 bytes (a 32-bit byte offset) and, at tier B, modulo 2^31 elements is
      * inside the table (a wrapped READ returns data, it does not fault), and
      * either the NaN fill outside every view, or a place inside a view that is not the same (view, row, column 0): another row or
        another matrix, whose hashed values differ from this row's.
    So a wrapped read changes the result and a wrapped write leaves the NaN fill where the result is expected."""
    table = meta_table(tier)
    lay = table.layout(n, pitch_rows)
    views = [lay.take(d, dt) for dt in DTYPES for d in (104, 147)]
    if strided:
        views += [lay.take(147, torch.float32, rows=strided[0], step=strided[1]), lay.take(11, torch.float32)]
    row_bytes = lay.ld * 4
    for v in views:
        e = 2 if v.dtype == torch.bfloat16 else 4
        step = v.row_bytes // row_bytes
        checked = 0
        for r, off in enumerate(v.elem_offsets()):
            if off <= table.threshold:
                continue
            checked += 1
            true_byte = v.byte_col + r * v.row_bytes
            assert true_byte + v.t.shape[1] * e <= table.flat.numel() * 4
            for modulus in (2 ** 32 * e, 2 ** 32) + ((2 ** 31 * e,) if tier == "B" else ()):
                if true_byte < modulus:
                    continue                                               # an index of this width does not wrap here
                alias = true_byte % modulus
                assert 0 <= alias < true_byte and alias + v.t.shape[1] * e <= table.flat.numel() * 4
                kind, q, w = lay.alias_target(v, r, modulus)
                if kind == "row":
                    # the byte lies in view w at table row q: its row of w, and the column inside it
                    landed = (id(w), q // (w.row_bytes // row_bytes), alias % row_bytes - w.byte_col)
                    assert landed != (id(v), r, 0), (r, modulus)
                    assert q != r * step                                    # never this row's own place in the table
                else:
                    assert w is None
        assert checked >= 1


@pytest.mark.parametrize("tier", list(TIERS))
@pytest.mark.parametrize("n", NS + (257, 1031))
def test_default_pitch_puts_several_rows_beyond_the_threshold(tier, n):
    table = meta_table(tier)
    lay = table.layout(n, pitch_rows=default_pitch_rows(n))
    assert (n - 1) * lay.ld + ZONE <= table.flat.numel()
    for dt in DTYPES:
        v = lay.take(147, dt)
        assert v.far_rows(table.threshold) >= n // 50 + 1
        assert v.elem_offsets()[-1] + 147 <= table.flat.numel() * (2 if dt == torch.bfloat16 else 1)


def test_strided_rows_for_the_kmeans_centres():
    """k centres as every s-th row of a layout whose pitch is computed for (k - 1) s + 1 rows: the last centre and the last row of
    the n-row matrix next to it both lie beyond the threshold"""
    for tier in TIERS:
        table = meta_table(tier)
        n, k = 1031, 64
        s = (n - 1) // (k - 1)
        lay = table.layout(n, pitch_rows=(k - 1) * s + 1)
        x, c = lay.take(147), lay.take(147, rows=k, step=s)
        assert x.elem_offsets()[-1] > table.threshold and c.elem_offsets()[-1] > table.threshold
        assert c.t.stride(0) == s * lay.ld and c.t.shape == (k, 147)
        assert x.byte_col + x.width_bytes <= c.byte_col
        with pytest.raises(ValueError):
            lay.take(8, rows=k, step=s + 1)

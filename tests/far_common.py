"""Shared by test_far_layout_cpu.py and test_gpu_far_offsets.py: the layout arithmetic of the far-offset tests.  No GPU code: the
table wraps whatever flat float32 tensor it is given (the CPU test hands it a `device="meta"` tensor, which has a size and no memory).

Every entry point of the library takes a row pitch, so a row whose element offset does not fit in 32 bits needs a large PITCH, not
many rows: one flat allocation of a little over 2^32 float32 elements is viewed as [n, ld] with (n - 1) * ld > 2^32, and a test's
matrices are column ranges of that view -- n x d values each, whatever ld is.  The same bytes viewed as bfloat16 give the bf16
matrices: both views of a row start at the same BYTE, so a float32 view and a bfloat16 view handed out for one test cannot overlap,
and a bf16 row's element offset is twice the float32 one.

The whole table is filled once with FILL32: a NaN as float32 and as two bfloat16 (0x7FC0 each).  A kernel that wraps an offset then
reads a NaN or another row's values, or leaves the NaN where its result is expected; a write that went astray shows up as a word of
the table that is not FILL32 after the test has re-filled its own views."""
import torch

ZONE = 12288                      # float32 columns of a row that tests are handed: 16 hops of 512 columns plus outputs
ZONE_BYTES = ZONE * 4
ALIGN_BYTES = 32                  # every view starts, and ends, at a multiple of this within its row: 8 float32 / 16 bfloat16
SLACK = 1 << 27                   # elements the table holds beyond the threshold: the rounding of the pitch, the layouts whose pitch
                                  # is computed for fewer rows than they have (k-means centres), the zone of the last row
FILL32 = 0x7FC07FC0               # float32 NaN; as two bfloat16 0x7FC0, 0x7FC0: the quiet NaN
GIB = 1 << 30
# tier -> (free device memory it needs, element offset the last row of every matrix exceeds)
TIERS = {"A": (24 * GIB, 1 << 32),    # catches signed and unsigned 32-bit element offsets
         "B": (12 * GIB, 1 << 31)}    # signed ones only


def round_up(x, m):
    return (x + m - 1) // m * m


def far_pitch(n, elems_threshold, multiple=8):
    """the smallest pitch, a multiple of `multiple`, with (n - 1) * pitch > elems_threshold"""
    if n < 2:
        raise ValueError("a far pitch needs at least two rows")
    return round_up(-(-(elems_threshold + 1) // (n - 1)), multiple)


def default_pitch_rows(n):
    """The row count the GPU tests compute a layout's pitch for: 2 % fewer rows than the matrix has, so that not one but n // 50 + 1
    rows of every float32 matrix start beyond the threshold (at tier A: beyond what an unsigned 32-bit element offset holds).  The
    table then ends 2 % beyond the threshold, inside SLACK."""
    return n - n // 50


def table_elems(tier):
    """float32 elements of the one allocation of a tier: 17.7 GB (A), 9.1 GB (B)"""
    return TIERS[tier][1] + SLACK


def pick_tier(free_bytes):
    """"A", "B" or None (too little memory: the caller skips and says how much there was)"""
    for tier in ("A", "B"):
        if free_bytes >= TIERS[tier][0]:
            return tier
    return None


def esize(dtype):
    return 2 if dtype == torch.bfloat16 else 4


class FarView:
    """one matrix handed out by a FarLayout: `t` (the strided view), and where its rows start"""

    def __init__(self, t, byte_col, width_bytes, row_bytes, rows, dtype):
        self.t, self.byte_col, self.width_bytes, self.row_bytes, self.rows, self.dtype = t, byte_col, width_bytes, row_bytes, rows, dtype

    def byte_offsets(self):
        return [self.byte_col + r * self.row_bytes for r in range(self.rows)]

    def elem_offsets(self):
        e = esize(self.dtype)
        return [b // e for b in self.byte_offsets()]

    def far_rows(self, threshold):
        """rows whose first element lies beyond `threshold` elements of the view's dtype"""
        return sum(1 for o in self.elem_offsets() if o > threshold)


class FarLayout:
    """The table as [n, ld] float32 (and [n, 2 ld] bfloat16 over the same bytes), handing out disjoint column ranges of [0, ZONE).
    pitch_rows: the pitch is computed as if the matrix had that many rows (fewer than n: the last of `pitch_rows` rows taken at a
    row step is then beyond the threshold too, see take(step=))."""

    def __init__(self, table, n, pitch_rows=None):
        self.table, self.n = table, n
        self.ld = far_pitch(pitch_rows or n, table.threshold, 8)
        self.cursor = 0                                                   # bytes of the zone handed out so far
        self.views = []
        if (n - 1) * self.ld + ZONE > table.flat.numel():
            raise ValueError(f"{n} rows on a pitch of {self.ld} do not fit the table")

    def take(self, d, dtype=torch.float32, rows=None, step=1):
        """[rows, d] view (default: all n rows) of `dtype` whose row i is table row i * step, in the next free columns"""
        e = esize(dtype)
        rows = self.n if rows is None else rows
        if rows < 1 or (rows - 1) * step > self.n - 1:
            raise ValueError("rows beyond the layout")
        width = round_up(max(d, 1) * e, ALIGN_BYTES)
        if self.cursor + width > ZONE_BYTES:
            raise ValueError("the zone is full: nothing is handed out at or beyond ZONE")
        row_bytes = step * self.ld * 4
        flat = self.table.flat if dtype == torch.float32 else self.table.flat.view(dtype)
        t = torch.as_strided(flat, (rows, d), (row_bytes // e, 1), self.cursor // e)
        v = FarView(t, self.cursor, width, row_bytes, rows, dtype)
        self.cursor += width
        self.views.append(v)
        return v

    def refill(self):
        """every view handed out holds FILL32 again, over its whole aligned width; the zone is free again"""
        words = self.table.flat.view(torch.int32)
        for v in self.views:
            torch.as_strided(words, (v.rows, v.width_bytes // 4), (v.row_bytes // 4, 1), v.byte_col // 4).fill_(FILL32)
        self.views, self.cursor = [], 0

    def alias_target(self, v, r, modulus_bytes):
        """where row r of view v lands when its BYTE offset is taken modulo `modulus_bytes` (2^34 for a 32-bit float32 element
        offset, 2^33 for a bfloat16 one, 2^32 for a 32-bit byte offset): ("row", q, view) when the byte lies inside a view of
        table row q, else ("fill", q, None) -- the NaN fill outside every view"""
        b = (v.byte_col + r * v.row_bytes) % modulus_bytes
        q, c = divmod(b, self.ld * 4)
        for w in self.views:
            if w.byte_col <= c < w.byte_col + w.width_bytes and q % (w.row_bytes // (self.ld * 4)) == 0 \
                    and q // (w.row_bytes // (self.ld * 4)) < w.rows:
                return "row", q, w
        return "fill", q, None


class FarTable:
    """flat: a 1-D float32 tensor of table_elems(tier) elements; threshold: TIERS[tier][1]"""

    def __init__(self, flat, threshold):
        if flat.dim() != 1 or flat.dtype != torch.float32:
            raise TypeError("the table is one flat float32 tensor")
        self.flat, self.threshold = flat, threshold

    def layout(self, n, pitch_rows=None):
        return FarLayout(self, n, pitch_rows)

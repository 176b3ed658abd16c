"""Shared by the row-register aggregator tests (test_agg_rows_cpu.py, test_gpu_agg_variants.py) and, for the statements at the
end, by every GPU test module that states the same reference (test_gpu_parity.py, test_gpu_bf16.py, test_gpu_bf16_agg.py,
test_gpu_far_offsets.py); no GPU and no torch needed to import it (the statements import numpy / torch / the oracle when called).

Restatements, each made ONCE here, of what the library (csrc/sgl_core.cpp) decides on its own for the kernels that keep the hop
rows of a node in registers:
  * pick_lpr / pick_row_layout   the lane layout (lanes per row, 16-byte chunks per lane) for a row width and hop count
                                 (sgl::pick_lpr / sgl::row_layout)
  * hmax_of                      the hop capacity an instance is compiled for (sgl::row_instance)
  * expected_kernel              the template instance an entry point launches, or None where it takes its general path
  * compiled_variants            every template instance the launch tables can reach
plus the parser of these kernels' names as a profiler reports them, and the tuning keys that enter the rule."""
import contextlib
import functools
import re

from spmm_order_common import parse_template_args

# family -> kernel name in csrc/sgl_aggregate.hip
KERNELS = {"rowdot_reg": "hop_rowdot_reg_kernel", "nafs": "nafs_fused_kernel", "gate": "gate_fused_kernel",
           "recursive": "recursive_fused_kernel", "rowdot2": "hop_rowdot2_reg_kernel", "prefix": "nafs_prefix_kernel"}
FAMILIES = tuple(KERNELS)
_NAME = re.compile("(" + "|".join(KERNELS.values()) + ")")
_FAMILY_OF = {v: k for k, v in KERNELS.items()}
N_ARGS = {"rowdot_reg": 4, "nafs": 3, "gate": 3, "recursive": 3, "rowdot2": 3, "prefix": 2}

TUNING_KEYS = ("row_lpr32x2", "row_narrow_groups", "row_whole_lines")
TUNING_DEFAULTS = {"row_lpr32x2": 1, "row_narrow_groups": 1, "row_whole_lines": 1}
TUNING_VALUES = {"row_lpr32x2": (0, 1), "row_narrow_groups": (0, 1, 2, 3), "row_whole_lines": (0, 1)}

MAX_REG_HOPS = 16                 # "H <= 16, d <= 512": the entry points' test for the register-resident kernels
MAX_REG_WIDTH = 512

WIDE_LAYOUTS = ((8, 1), (16, 1), (32, 1), (64, 1), (32, 2), (64, 2))      # with_row_instance of csrc/sgl_rows.h: hop counts up to 16
NARROW_16X3 = (16, 3)                                                       # up to 12
NARROW_8X5 = (8, 5)                                                         # up to 6, hop_rowdot2_reg_kernel only


def pick_lpr(d, vec):
    """pick_lpr: the smallest of 8 / 16 / 32 / 64 lanes that covers ceil(d / vec) lane accesses (64 when none does)"""
    lanes = (d + vec - 1) // vec
    lpr = 8
    while lpr < lanes and lpr < 64:
        lpr <<= 1
    return lpr


def pick_row_layout(d, n_hops, allow_8x5=False, tuning=None):
    """pick_row_layout -> (LPR, CH).  tuning = {key: value}, missing keys at their defaults."""
    t = tuning or {}
    return _row_layout(d, n_hops, bool(allow_8x5), t.get("row_lpr32x2", TUNING_DEFAULTS["row_lpr32x2"]),
                       t.get("row_narrow_groups", TUNING_DEFAULTS["row_narrow_groups"]))


@functools.lru_cache(maxsize=None)
def _row_layout(d, n_hops, allow_8x5, lpr32x2, mode):
    lpr = pick_lpr(d, 4)
    ch = 2 if d > lpr * 4 else 1
    if lpr == 64 and ch == 1 and d > 128 and lpr32x2 != 0:                    # 2 rows per wavefront
        lpr, ch = 32, 2
    if mode != 0 and d <= lpr * 4 * ch:
        slots = (d + 3) // 4
        for lanes, chunks, most_hops in ((16, 3, 12), (8, 5, 6)):
            idle = lanes * chunks - slots
            if ((mode == 2 or not allow_8x5) and lanes == 8) or (mode == 3 and lanes == 16):
                continue
            if idle >= 0 and n_hops <= most_hops and 2 * idle <= lpr * ch - slots:
                lpr, ch = lanes, chunks
    return lpr, ch


def hmax_of(layout, n_hops):
    """sgl::row_instance: the even hop capacity of the instance that serves n_hops in this layout; None where the
    table of the layout has no such row (pick_row_layout never sends such a hop count there)"""
    most = 6 if layout == NARROW_8X5 else 12 if layout == NARROW_16X3 else 16
    if n_hops < 1 or n_hops > most:
        return None
    return max(2, (n_hops + 1) // 2 * 2)


def expected_kernel(family, d, n_hops, tuning=None, g_unaligned=False, aligned=True):
    """(family, (LPR, CH, HMAX[, GU])) -- (family, (LPR, CH)) for "prefix" -- of the one kernel of `family` that its entry point
    launches for hops of width d, or None where the entry point takes its general path (or refuses): more than 16 hops, d > 512,
    or rows that are not 16-byte aligned with pitches that are multiples of 4 floats (aligned=False).  g_unaligned ("rowdot_reg"
    only): dOut is only dword-aligned, the GU instance reads it."""
    if family not in KERNELS:
        raise ValueError(family)
    if not aligned or d < 1 or d > MAX_REG_WIDTH:
        return None
    if family == "prefix":                                                   # any hop count: the layout is picked for one hop
        return family, pick_row_layout(d, 1, False, tuning)
    if n_hops < 1 or n_hops > MAX_REG_HOPS:
        return None
    lay = pick_row_layout(d, n_hops, family == "rowdot2", tuning)
    if d > lay[0] * 4 * lay[1]:
        return None
    hm = hmax_of(lay, n_hops)
    if hm is None:
        raise AssertionError(f"layout {lay} picked for {n_hops} hops it is not compiled for")
    return family, lay + ((hm, 1 if g_unaligned else 0) if family == "rowdot_reg" else (hm,))


def compiled_variants(family):
    """every instance the launch tables reach: the six wide layouts x HMAX 2, 4 .. 16, 16 x 3 x HMAX 2 .. 12, for "rowdot2" also
    8 x 5 x HMAX 2, 4, 6; "rowdot_reg" x GU; "prefix" is instantiated over the layout alone (never 8 x 5)"""
    if family == "prefix":
        return set(WIDE_LAYOUTS) | {NARROW_16X3}
    out = {lay + (hm,) for lay in WIDE_LAYOUTS for hm in range(2, 17, 2)}
    out |= {NARROW_16X3 + (hm,) for hm in range(2, 13, 2)}
    if family == "rowdot2":
        out |= {NARROW_8X5 + (hm,) for hm in (2, 4, 6)}
    if family == "rowdot_reg":
        out = {v + (gu,) for v in out for gu in (0, 1)}
    return out


def parse_agg_kernel_name(name):
    """(family, template arguments) from the name of an instance of one of the six kernels, demangled
    (`void (anonymous namespace)::hop_rowdot_reg_kernel<16, 3, 6, (bool)1>(...)`, `... true>`) or mangled
    (`_ZN12_GLOBAL__N_121hop_rowdot_reg_kernelILi16ELi3ELi6ELb1EEEv...`); None for any other kernel.  A name of one of the six
    without its full template arguments is an error: the tests identify instances by them."""
    m = _NAME.search(name)
    if not m:
        return None
    family = _FAMILY_OF[m.group(1)]
    args = parse_template_args(name[m.end():])
    if args is None or len(args) != N_ARGS[family]:
        raise ValueError(f"unexpected template arguments in {name!r}")
    return family, tuple(args)


# ---- a reference shared by test_gpu_parity.py and test_gpu_agg_variants.py --------------------------------------------------------
def recursive_step_by_step(feats, weight, bias, cond=None):
    """the reference's loop as written (iterate_learnable_weighted_message_op.py:28-51), any dtype, plain torch.  cond (a dict):
    receives the condition magnitudes of the Linear's gradients -- the sums of the ABSOLUTE terms of weight.grad and bias.grad"""
    import torch
    acc, weights = feats[0], None
    for i in range(len(feats)):
        inp = torch.hstack((feats[i], acc))
        z = inp @ weight.view(-1, 1) + bias
        if cond is not None and z.requires_grad:
            def hook(g_, inp=inp.detach()):
                cond["bias"] = cond.get("bias", 0) + g_.abs().sum()
                cond["weight"] = cond.get("weight", 0) + g_.abs().t() @ inp.abs()
            z.register_hook(hook)
        score = torch.sigmoid(z)
        weights = score if weights is None else torch.hstack((weights, score))
        weights = torch.softmax(weights, dim=1)
        acc = sum(weights[:, j:j + 1] * feats[j] for j in range(i + 1))
    return acc, weights


# ---- the case list of test_gpu_agg_variants.py -------------------------------------------------------------------------------
N_ROWS = 77                       # no multiple of the 4 .. 32 rows a block holds: the last block is partial in every layout
LPR64X1 = {"row_lpr32x2": 0, "row_narrow_groups": 0}
# (layout, width, tuning): one width per layout for the sweep over all hop counts; at 147 the hop counts 13 .. 16 go to (32, 2)
HOP_SWEEP = (((8, 1), 29, {}), ((16, 1), 61, {}), ((32, 1), 100, {}), ((16, 3), 147, {}), ((32, 2), 255, {}), ((64, 2), 509, {}),
             ((64, 1), 250, LPR64X1))
WIDTH_8X5 = 157                   # hop_rowdot2_reg_kernel only: 8 x 5 for 1 .. 6 hops, 16 x 3 from 7
WIDTH_16X3_ONLY = 177             # ... which therefore needs a row 8 x 5 cannot hold (> 160) to run 16 x 3 with 1 .. 6 hops
# both sides of every layout boundary, and d % 4 in {1, 2, 3}
WIDTH_SWEEP = (1, 3, 4, 32, 33, 64, 65, 128, 129, 160, 161, 192, 193, 256, 257, 511, 512)
WIDTH_SWEEP_HOPS = (5, 6)
PREFIX_HOPS = (1, 5, 17, 40)


def case_list(family):
    """[(n_rows, d, n_hops, tuning)] of one family, duplicates removed, in a fixed order"""
    out = []
    if family == "prefix":
        for _, d, tuning in HOP_SWEEP:
            out += [(N_ROWS, d, h, tuning) for h in PREFIX_HOPS] + [(1, d, 5, tuning)]
        return out
    for _, d, tuning in HOP_SWEEP:
        out += [(N_ROWS, d, h, tuning) for h in range(1, 17)] + [(1, d, 5, tuning)]
    if family == "rowdot2":
        out += [(N_ROWS, WIDTH_8X5, h, {}) for h in range(1, 8)] + [(1, WIDTH_8X5, 5, {})]
        out += [(N_ROWS, WIDTH_16X3_ONLY, h, {}) for h in range(1, 7)] + [(1, WIDTH_16X3_ONLY, 5, {})]
    for h in WIDTH_SWEEP_HOPS:
        out += [(N_ROWS, d, h, {}) for d in WIDTH_SWEEP]
        out += [(N_ROWS, 147, h, {"row_narrow_groups": m}) for m in (0, 2, 3)]
    seen, uniq = set(), []
    for c in out:
        key = (c[0], c[1], c[2], tuple(sorted(c[3].items())))
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return uniq


@contextlib.contextmanager
def tuned(**kw):
    """the three layout keys set as given (the others at their defaults) for the block, restored on exit"""
    from sgl_amd import _lib
    saved = {k: _lib.get_tuning(k) for k in TUNING_KEYS}
    try:
        for k in TUNING_KEYS:
            _lib.set_tuning(k, kw.get(k, TUNING_DEFAULTS[k]))
        yield
    finally:
        for k, v in saved.items():
            _lib.set_tuning(k, v)


# ---- statements shared by several GPU test modules: each is made ONCE here ----------------------------------------------------------
PARITY_TOL = 1e-5                 # the project's parity contract
BIAS = 0.37                       # the gate bias of test_gpu_agg_variants.py and test_gpu_far_offsets.py


def t64(x):
    import numpy as np
    import torch
    return torch.from_numpy(np.asarray(x)).double()


def t32(x):
    import numpy as np
    import torch
    return torch.from_numpy(np.asarray(x)).float()


def vector(d, seed, scale):
    import numpy as np
    from inputs import hash_matrix
    return np.ascontiguousarray(hash_matrix(1, d, seed=seed)[0] * np.float32(scale)).astype(np.float32)


def gate_reference(host, v, dt):
    """(out, W, G) of the learnable gate over the host hops with the Linear v and the bias BIAS, plain torch in dtype dt"""
    import torch
    ff = [torch.from_numpy(x).to(dt) for x in host]
    vv = torch.from_numpy(v).to(dt)
    g = torch.sigmoid(torch.stack([f @ vv + torch.tensor(BIAS, dtype=torch.float32).to(dt) for f in ff], dim=1))
    w = torch.softmax(g, dim=1)
    return sum(w[:, h:h + 1] * ff[h] for h in range(len(ff))), w, g


def rne(a):
    """the one definition of rounding to bfloat16: torch's round to nearest even on the CPU"""
    import numpy as np
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def bits32(a):
    import numpy as np
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits32(got, want):
    """32-bit patterns equal; where the expected value is a NaN the result must be a NaN (payloads are not compared)"""
    import numpy as np
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits32(got)[~nan], bits32(want)[~nan]))


def reduce_statement(kind, wide, w):
    """hop_reduce_kernel's order in numpy float32: sum / mean start from 0 + X_s, mean ends with one true division, the weighted
    sum is a rounded product, then an add, max / min propagate NaN"""
    import numpy as np
    with np.errstate(all="ignore"):
        if kind in ("sum", "mean"):
            acc = np.float32(0.0) + wide[0]
            for x in wide[1:]:
                acc = acc + x
            return acc / np.float32(len(wide)) if kind == "mean" else acc
        if kind == "wsum":
            acc = wide[0] * w[0]
            for h in range(1, len(wide)):
                acc = acc + wide[h] * w[h]
            return acc
        acc = wide[0]
        for x in wide[1:]:
            acc = (np.maximum if kind == "max" else np.minimum)(acc, x)
        return acc


def long_row_graph(n=1500, seed=5, unit_rows=False):
    """power-law rows plus three huge rows (1400, 900 and 1499 non-zeros) and some empty ones (canonical CSR, not symmetric).
    unit_rows: the values are divided by the square root of their row's length, so that row sums of |a| are of order 1 and several
    hops stay of order 1 (the bfloat16 tests)"""
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    deg = np.minimum(rng.lognormal(1.2, 1.0, n).astype(np.int64), 200)
    deg[rng.integers(0, n, 60)] = 0
    deg[[3, 700, n - 1]] = [1400, 900, 1499]
    rows, cols = [], []
    for i in range(n):
        c = np.sort(rng.choice(n, int(deg[i]), replace=False))
        rows.append(np.full(len(c), i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.uniform(-1, 1, len(rows))
    vals = (vals / np.sqrt(np.maximum(deg[rows], 1)) if unit_rows else vals).astype(np.float32)
    a = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    a.sort_indices()
    return a


def sig_mix(bits, r):
    """the mix of sgl_col_signature_f32's definition, sig[c] = sum_r mix(bits(X[r, c]), r) mod 2^64, in numpy uint64"""
    import numpy as np
    with np.errstate(over="ignore"):
        h = (bits.astype(np.uint64) ^ (r.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))) * np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(31)
        h *= np.uint64(0x94D049BB133111EB)
        return h ^ (h >> np.uint64(29))


def bf16_fast_order_bound(a64, ptr, col, val, xin, got):
    """(err, bound) per element of one bfloat16 fast-order product from the stored input xin (float32 values of a bf16 matrix):
    T = the float64 product, R = the oracle (float32, strict order), G = got widened;  b = max(2 max|R - T|, TRUTH_FLOOR max|T|)
    (truth_report's bound);  |G - T| <= 2^-8 |T| + (1 + 2^-8) b: RNE to 8 significant bits errs by at most 2^-8 relative, the
    float32 sum in another order gets the standing factor 2"""
    import numpy as np
    import oracle
    T = a64 @ xin.astype(np.float64)
    R = oracle.oracle_spmm(ptr, col, val, xin).astype(np.float64)
    G = np.asarray(got).astype(np.float64)
    b = max(2.0 * np.abs(R - T).max(), oracle.TRUTH_FLOOR * np.abs(T).max())
    return np.abs(G - T), 2.0 ** -8 * np.abs(T) + (1.0 + 2.0 ** -8) * b

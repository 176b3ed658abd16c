"""Shared by the SpMM summation-order tests (test_spmm_order_cpu.py, test_gpu_spmm_order.py); no GPU needed to import it.

Three restatements, each made ONCE here, of things the library decides on its own:
  * default_long_row_nnz   where sgl_csr_create cuts long rows when it is not told (sgl::default_long_row_nnz, csrc/sgl_core.cpp)
  * dispatch               which kernel template spmm_impl / spmm_slice launch for a call: the lane width in csrc/sgl_spmm.hip and
                           sgl_spmm_bf16.hip, the layout in sgl::spmm_layout (csrc/sgl_core.cpp)
  * compiled_variants      every template instance the launch tables of the two files can reach
(the first two are compared with the library's own answers without a GPU in test_spmm_order_cpu.py)
plus the parser of kernel names as a profiler reports them, and the test graphs."""
import re

import numpy as np
import scipy.sparse as sp


def default_long_row_nnz(nnz):
    """sgl::default_long_row_nnz, csrc/sgl_core.cpp: `nnz < (1 << 18) ? 32 : nnz < (1 << 20) ? 128 : nnz < (1 << 22) ? 512 : 2048`"""
    nnz = int(nnz)
    return 32 if nnz < (1 << 18) else 128 if nnz < (1 << 20) else 512 if nnz < (1 << 22) else 2048


def cut_rule(rowptr, long_row_nnz):
    """the pieces of every row that is cut: [(row, begin, len)], rows ascending, a row's pieces in storage order.  A row with
    more than long_row_nnz non-zeros is cut into pieces of long_row_nnz from its start; <= 0 never cuts."""
    out = []
    if long_row_nnz <= 0:
        return out
    for r in range(len(rowptr) - 1):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        if e - b > long_row_nnz:
            out += [(r, p, min(long_row_nnz, e - p)) for p in range(b, e, long_row_nnz)]
    return out


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def uniform_degree_graph(n, lo, hi, seed, extra=()):
    """canonical CSR (sorted, unique columns, not symmetric): degrees uniform lo..hi, 40 empty rows, three rows of >= 900
    non-zeros, rows of exactly 32 / 33 / 128 / 129 non-zeros (the cut thresholds and one more), values uniform(-1, 1) / sqrt(deg)"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(lo, hi + 1, n)
    deg[rng.choice(np.arange(20, n - 20), 40, replace=False)] = 0
    deg[[3, n // 2, n - 1]] = [1100, 900, n - 1]
    deg[[10, 11, 12, 13]] = [32, 33, 128, 129]
    for r, k in extra:
        deg[r] = k
    cols = [np.sort(rng.choice(n, int(k), replace=False)) for k in deg]
    rows = np.repeat(np.arange(n), deg)
    vals = (rng.uniform(-1, 1, len(rows)) / np.sqrt(np.maximum(deg[rows], 1))).astype(np.float32)
    a = sp.csr_matrix((vals, np.concatenate(cols), np.concatenate([[0], np.cumsum(deg)])), shape=(n, n))
    assert a.has_canonical_format
    return a


def medium_graph():
    return uniform_degree_graph(1500, 8, 47, seed=11)


def dense_graph():
    return uniform_degree_graph(1200, 20, 99, seed=12)


# ---- kernel names -----------------------------------------------------------------------------------------------------------
_NAME = re.compile(r"spmm_(bf16_)?kernel")


def parse_template_args(rest):
    """the integer template arguments that follow a kernel's name (shared with agg_rows_common.py): `<4, 64, (bool)1, false>(...)`
    of a demangled name or `ILi4ELi64ELb1ELb0EEEv...` of a mangled one; None when there are none"""
    if rest.startswith("<"):
        inner = rest[1:rest.index(">")]
        args = []
        for tok in inner.split(","):
            tok = tok.strip()
            tok = tok[tok.rfind(")") + 1:] if ")" in tok else tok           # `(bool)1`, `(int)4`
            args.append(1 if tok == "true" else 0 if tok == "false" else int(tok))
        return args
    mm = re.match(r"I((?:L[a-z]\d+E)+)E", rest)
    if not mm:
        return None
    return [int(v) for v in re.findall(r"L[a-z](\d+)E", mm.group(1))]


def parse_kernel_name(name):
    """("bf16", (BV, GROUP, NCH, U)) / ("f32", (VEC, GROUP, NCH, U, NT)) from the name of an spmm_bf16_kernel / spmm_kernel
    instance, None for any other kernel (the fix-up kernels included).  Accepts the demangled form
    `... spmm_kernel<4, 64, 1, 16, false, false>(...)` and the mangled one `_ZN..11spmm_kernelILi4ELi64ELi1ELi16ELb0ELb0EEEv...`."""
    m = _NAME.search(name)
    if not m:
        return None
    args = parse_template_args(name[m.end():])
    if args is None:
        return None
    if m.group(1):
        if len(args) != 4:
            raise ValueError(f"unexpected template arguments in {name!r}")
        return "bf16", tuple(args)
    if len(args) != 6 or args[5] != 0:                                       # MULTI (replicas) is not part of these tests
        raise ValueError(f"unexpected template arguments in {name!r}")
    return "f32", tuple(args[:5])


# ---- dispatch ----------------------------------------------------------------------------------------------------------------
LAYOUTS = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))      # (GROUP, NCH): launch_group of both files


def unroll_of(group, nch, ulevel):
    """sgl::unroll_of (csrc/sgl_common.h), the template argument of launch_u in both files (sgl_spmm.hip has level 3 in addition):
    gathers in flight per lane"""
    uh = 8 if nch == 1 else 4 if nch == 2 else 2
    if ulevel == 2:
        return uh * 2 if nch == 1 else uh
    if ulevel == 3:
        return 32 if (nch == 1 and group == 64) else uh
    return uh // 2 if ulevel == 0 else uh


def compiled_variants(dtype):
    """every instance the launch tables reach.  bf16 (sgl_spmm_bf16.hip, launch_variant / launch_u / launch_group / the bv switch
    of spmm_slice): BV in {8, 4, 2, 1} x the six layouts x levels 0..2.  fp32 (sgl_spmm.hip, launch_nt / launch_u / launch_group /
    the vec switch of spmm_slice): VEC in {4, 2, 1} x the six layouts x levels 0..3 x NT."""
    out = set()
    if dtype == "bf16":
        for w in (8, 4, 2, 1):
            for g, c in LAYOUTS:
                for lv in (0, 1, 2):
                    out.add((w, g, c, unroll_of(g, c, lv)))
    else:
        for w in (4, 2, 1):
            for g, c in LAYOUTS:
                for lv in (0, 1, 2, 3):
                    for nt in (0, 1):
                        out.add((w, g, c, unroll_of(g, c, lv), nt))
    return out


TUNING_KEYS = ("spmm_group", "spmm_unroll", "spmm_waves", "spmm_xcd_remap", "spmm_nt", "spmm_vec")
TUNING_DEFAULTS = {"spmm_group": 0, "spmm_unroll": 0, "spmm_waves": 0, "spmm_xcd_remap": 1, "spmm_nt": 0, "spmm_vec": 0}
TUNING_VALUES = {"spmm_group": (0, 8, 16, 32, 64), "spmm_unroll": (0, 1, 2, 3, 4), "spmm_waves": (0, 1, 2, 4),
                 "spmm_xcd_remap": (0, 1), "spmm_nt": (0, 1), "spmm_vec": (0, 1, 2)}


def dispatch(dtype, d, ldx, ldy, x_ptr, y_ptr, strict, avg_nnz, tuning=None, acc=None):
    """[(c0, dc, variant)] per column slice of one sgl_spmm_f32 / sgl_spmm_bf16 (/ _acc_) call: spmm_impl and spmm_slice of
    csrc/sgl_spmm.hip and csrc/sgl_spmm_bf16.hip with sgl::spmm_layout of csrc/sgl_core.cpp restated.  Pitches in elements, pointers in bytes, avg_nnz = nnz / n_rows,
    acc = (ldacc, acc_ptr) of the fused aggregate, tuning = {key: value} (missing keys at their defaults).
    variant = (BV, GROUP, NCH, U) for "bf16", (VEC, GROUP, NCH, U, NT) for "f32"; R = 64 // GROUP."""
    t = dict(TUNING_DEFAULTS)
    t.update(tuning or {})
    bf16 = dtype == "bf16"
    esize = 2 if bf16 else 4
    w = 1
    for cand in ((8, 4, 2) if bf16 else (4, 2)):                     # pick_bv / pick_vec
        if d % cand == 0 and ldx % cand == 0 and ldy % cand == 0 and x_ptr % (esize * cand) == 0 and y_ptr % (esize * cand) == 0:
            w = cand
            break
    vcap = t["spmm_vec"]
    if bf16:
        if acc is not None:
            ldacc, ap = acc
            if w >= 4 and not (ldacc % 4 == 0 and ap % 16 == 0):
                w = 2
            if w == 2 and not (ldacc % 2 == 0 and ap % 8 == 0):
                w = 1
        if vcap in (1, 2) and vcap < w:
            w = vcap
    else:
        if vcap in (1, 2) and vcap < w:
            w = vcap
        if acc is not None:
            ldacc, ap = acc
            if w == 4 and not (ldacc % 4 == 0 and ap % 16 == 0):
                w = 2 if (ldacc % 2 == 0 and ap % 8 == 0 and d % 2 == 0) else 1
            if w == 2 and not (ldacc % 2 == 0 and ap % 8 == 0):
                w = 1
    out = []
    max_cols = 64 * 4 * w
    for c0 in range(0, d, max_cols):
        dc = min(max_cols, d - c0)
        lanes = dc // w
        group, nch = 64, 1
        if lanes > 64:
            need = (lanes + 63) // 64
            nch = need if need <= 2 else 4
        elif not strict and lanes <= 16:
            group = 8
            while group < lanes:
                group <<= 1
        forced = t["spmm_group"]
        if not strict and forced in (8, 16, 32, 64) and nch == 1 and forced >= lanes:
            group = forced
        ulevel = 2 if (group == 64 and nch == 1) else 1
        if nch == 1:
            if group == 64:
                if avg_nnz < 12.0:
                    ulevel = 0
                elif avg_nnz < 40.0:
                    ulevel = 1
            elif bf16 and avg_nnz >= 40.0:
                ulevel = 2
        un = t["spmm_unroll"]
        ulevel = {1: 0, 2: 2, 3: 1}.get(un, ulevel)
        if un == 4 and not bf16:
            ulevel = 3
        var = (w, group, nch, unroll_of(group, nch, ulevel))
        if not bf16:
            var += (1 if t["spmm_nt"] else 0,)
        out.append((c0, dc, var))
    return out

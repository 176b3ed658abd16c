"""Shared by test_degenerate_cpu.py and test_gpu_degenerate_rows.py (importable without a GPU): the aggregator family of
csrc/sgl_aggregate.hip / sgl_aggregate_bf16.hip / sgl_rows.h on non-finite, saturated and degenerate rows.

Stated ONCE here:
  * the inputs: 77 rows, one width per lane layout (agg_rows_common.HOP_SWEEP) at 2, 5 and 13 hops, three general paths, and the
    finite ill-conditioned regimes (NAFS at five scales with correlated / duplicate / negated hops, saturated gates);
  * the injections: ONE element of one hop replaced by NaN, +inf, -inf, 3e38 or -3e38;
  * the statements: plain torch / numpy on the CPU of the reference expressions, in float32 and float64, one per family;
  * the rule that compares a kernel with its statement.  It needs no tolerance:
      - an output entry whose float32 statement has the same bits on the clean and on the poisoned input is INDEPENDENT of the
        poisoned element, every other entry is TOUCHED;
      - independent entries of the kernel's output are bit-identical to the kernel's own clean run;
      - on touched entries the NaN, +inf and -inf masks equal the float32 statement's;
      - touched entries that are finite go through oracle.truth_report against the float64 statement, restricted to them.

A family is a pair of functions over the same arguments (X: the hop list, p: the parameters, both torch tensors): `ref` is the
statement, `gpu` calls the wrapper of sgl_amd/device.py.  Both return {name: tensor}; gradients are taken by the same helper
(grads) through autograd on either side and are named "d<parameter>".  The row axis of an output is its last but one
([n, d], [n, H], [H, n, d]); the outputs listed in `reduced` are summed over the rows and have none."""
import collections

import numpy as np

import ensemble_common as ec
from agg_rows_common import BIAS, HOP_SWEEP, N_ROWS, expected_kernel, recursive_step_by_step, reduce_statement, vector

N = N_ROWS
ROWS = (0, 37, 76)
HOP_COUNTS = (2, 5, 13)
BF16_BIG = float(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0])          # the largest finite bfloat16
VALUES = (("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf")), ("+3e38", 3e38), ("-3e38", -3e38))
VALUES_BF16 = VALUES[:3] + (("+7F7F", BF16_BIG), ("-7F7F", -BF16_BIG))
ROUNDING = 2.0 ** -24               # one float32 rounding of a value near 1

Shape = collections.namedtuple("Shape", "tag d H tuning dense")
Injection = collections.namedtuple("Injection", "row hop col name value")


def shapes():
    """one width per lane layout x 2 / 5 / 13 hops (at 13 hops 147 moves to 32 x 2 and d = 29 has more hops than lanes: the array
    form of the gate and the recursion), then the three general paths: d = 600 (no kernel keeps the rows in registers), 17 hops,
    dense d = 147 tensors (rows not 16-byte aligned: the element path)"""
    out = [Shape(f"{lay[0]}x{lay[1]}", d, H, tuning, False) for lay, d, tuning in HOP_SWEEP for H in HOP_COUNTS]
    return out + [Shape("wide", 600, 5, {}, False), Shape("hops17", 100, 17, {}, False), Shape("dense", 147, 5, {}, True), ONLY_16X3]


# the two-part scores run 147 columns in their own 8 x 5 layout up to 6 hops: their 16 x 3 instances need a row 8 x 5 cannot hold
ONLY_16X3 = Shape("16x3-rowdot2", 177, 5, {}, False)


def sid(s):
    return f"{s.tag}-d{s.d}-H{s.H}"


def injections(shape, k, bf16=False):
    """15 of the 90 (row, hop, column, value) combinations for the k-th shape of a family's list: every value, every row, both hops
    and the three columns (0, d - 1, d // 2: at the wider layouts they fall into different lanes' chunks) in each block of 15, and
    all 90 combinations over six consecutive shapes.  i mod 30 <-> (value, row, hop) is a bijection (5, 3, 2 are coprime) and the
    column index (i // 30 + row) mod 3 completes it."""
    vals = VALUES_BF16 if bf16 else VALUES
    cols = (0, shape.d - 1, shape.d // 2)
    out = []
    for j in range(15):
        i = (15 * k + j) % 90
        name, value = vals[i % 5]
        out.append(Injection(ROWS[i % 3], (0, shape.H - 1)[i % 2], cols[(i // 30 + i) % 3], name, value))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
_HOPS = {}


def host_hops(d, H, bf16=False):
    """the hops of test_gpu_agg_variants.py: hop h = hash_matrix scaled by (1 - 0.04 h), row 1 of hop 0 zero, row 3 of every hop
    zero; bf16: rounded to bfloat16 (returned as the float32 values of the bfloat16 matrices)"""
    from inputs import hash_matrix
    have = _HOPS.setdefault((d, bf16), [])
    for h in range(len(have), H):
        x = np.ascontiguousarray((hash_matrix(N, d, seed=31 * d + h) * np.float32(1.0 - 0.04 * h)).astype(np.float32))
        if h == 0:
            x[1] = 0.0
        x[3] = 0.0
        if bf16:
            import torch
            x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
        have.append(x)
    return have[:H]


def poisoned(hops, inj):
    """the hop list with ONE element replaced (the other hops are shared, not copied)"""
    out = list(hops)
    x = hops[inj.hop].copy()
    x[inj.row, inj.col] = inj.value
    out[inj.hop] = x
    return out


def parameters(d, H):
    """every parameter any family reads, float32 numpy; the entries of COLUMNS have the feature columns as their last axis"""
    from inputs import hash_matrix
    w1 = vector(H, 3 * d + 1, 1.0)
    w1[np.abs(w1) < 0.05] = 0.25                                        # no weight is zero (0 * inf) or denormal
    lin = np.ascontiguousarray(hash_matrix(3, H, seed=5 * d + 4))
    lin[np.abs(lin) < 0.05] = 0.25
    lin[1, H - 1] = 0.0                                                 # a skipped term: what that hop holds must not reach output 1
    return {"w1": w1, "w2": np.ascontiguousarray((hash_matrix(N, H, seed=d + 7) + np.float32(1.5)) / np.float32(H)),
            "ws": np.ascontiguousarray(hash_matrix(N, 1, seed=d + 8)[:, 0]),
            "lin": lin, "v": vector(d, 7 * d + 1, 0.3), "wt": vector(2 * d, 11 * d + 3, 0.5 / d ** 0.5).reshape(2, d),
            "u": np.ascontiguousarray(hash_matrix(H, d, seed=17 * d + H) * np.float32(0.3)), "b": np.array([BIAS], np.float32),
            "gout": np.ascontiguousarray(hash_matrix(N, d, seed=5 * d + 2)), "gw": np.ascontiguousarray(hash_matrix(N, H, seed=5 * d + 3)),
            "ga": np.ascontiguousarray(hash_matrix(N, 1, seed=5 * d + 5)), "old": np.ascontiguousarray(hash_matrix(N, d, seed=3 * d + 9))}


COLUMNS = ("v", "wt", "u", "gout", "old")


def reversed_columns(hops, p):
    """the same problem with the feature columns in the opposite order"""
    return [np.ascontiguousarray(x[:, ::-1]) for x in hops], {k: (np.ascontiguousarray(a[..., ::-1]) if k in COLUMNS else a) for k, a in p.items()}


def unreverse(outs, d):
    return {k: (np.ascontiguousarray(a[..., ::-1]) if a.ndim and a.shape[-1] == d else a) for k, a in outs.items()}


# ---- autograd, the same on both sides --------------------------------------------------------------------------------------------
def leaves(X):
    return [x.detach().requires_grad_(True) for x in X]


def leaf(t):
    return t.detach().clone().requires_grad_(True)


def grads(pairs, wrt, X=None, inner=None):
    """{"d" + name: gradient} of sum <output, given gradient> with respect to the named parameters, and "dX" [H, n, d] for the hops;
    inner: an intermediate tensor whose gradient is returned as well, under "inner" (for the condition magnitudes)"""
    import torch
    loss = sum((o * g).sum() for o, g in pairs)
    params = list(wrt.values()) + list(X or []) + ([inner] if inner is not None else [])
    got = torch.autograd.grad(loss, params, allow_unused=True)
    got = [torch.zeros_like(t) if g is None else g for t, g in zip(params, got)]
    out = {"d" + k: g for k, g in zip(wrt, got)}
    if X:
        out["dX"] = torch.stack(got[len(wrt):len(wrt) + len(X)])
    if inner is not None:
        out["inner"] = got[-1]
    return out


def _np(X):
    return [x.detach().numpy() for x in X]


def _t(a, like):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(like.dtype)


# ---- the statements ----------------------------------------------------------------------------------------------------------------
def ref_reduce(kind):
    def ref(X, p):
        with np.errstate(all="ignore"):
            return {"out": _t(reduce_statement(kind, _np(X), p["w1"].numpy()), X[0])}
    return ref


def ref_select(kind):
    """max / min over the hops with the gradient torch sends to the selected hop"""
    def ref(X, p):
        import torch
        X = leaves(X)
        st = torch.stack(X)
        out = st.max(0)[0] if kind == "max" else st.min(0)[0]
        return {"out": out, **grads([(out, p["gout"])], {}, X)}
    return ref


def ref_lincomb(X, p):
    """out_k = sum_j lin[k, j] X_j from 0 in j order; a zero weight skips its term"""
    import torch
    outs = []
    for k in range(p["lin"].shape[0]):
        acc = torch.zeros_like(X[0])
        for j, x in enumerate(X):
            if float(p["lin"][k, j]) != 0.0:
                acc = acc + p["lin"][k, j] * x
        outs.append(acc)
    return {"out": torch.stack(outs)}


def ref_wsum1d(X, p):
    """one_dim_weighted_add: sum_h w[h] X_h, and dw[h] = sum over rows and columns of dOut X_h"""
    w = leaf(p["w1"])
    out = X[0] * w[0]
    for h in range(1, len(X)):
        out = out + X[h] * w[h]
    return {"out": out, **grads([(out, p["gout"])], {"w1": w})}


def ref_wsum2d(X, p):
    """two_dim_weighted_add: out[n] = sum_h W[n, h] X_h[n]; dW[n, h] = <dOut[n], X_h[n]>, dX_h = W[:, h] dOut"""
    X, w = leaves(X), leaf(p["w2"])
    out = sum(w[:, h:h + 1] * X[h] for h in range(len(X)))
    return {"out": out, **grads([(out, p["gout"])], {"w2": w}, X)}


def ref_scores(X, p):
    """P[n, h] = <X_h[n], v>; dv = sum_h X_h^T dP[:, h]"""
    import torch
    v = leaf(p["v"])
    P = torch.stack([x @ v for x in X], 1)
    return {"P": P, **grads([(P, p["gw"])], {"v": v})}


def scores2_args(H):
    """(mask, h0, h1) of test_gpu_agg_variants.py: two of every three hops and the last one in the reference part"""
    return (0xB6DB & ((1 << H) - 1)) | (1 << (H - 1)), (1 if H >= 3 else 0), H


def ref_scores2(X, p):
    """P[n, h - h0] = <X_h[n], v> and A[n] = sum_{j in mask} <X_j[n], U[j]>, with dv and dU"""
    import torch
    H = len(X)
    mask, h0, h1 = scores2_args(H)
    v, u = leaf(p["v"]), leaf(p["u"])
    P = torch.stack([X[h] @ v for h in range(h0, h1)], 1)
    A = sum(X[j] @ u[j] for j in range(H) if (mask >> j) & 1)[:, None]
    return {"P": P, "A": A, **grads([(P, p["gw"][:, h0:h1]), (A, p["ga"])], {"v": v, "u": u})}


def ref_colsum(shared):
    def ref(X, p):
        import torch
        return {"out": torch.stack([x.t() @ (p["ws"] if shared else p["w2"][:, h]) for h, x in enumerate(X)])}
    return ref


def ref_gate(X, p):
    """LearnableWeightedMessageOp 'gate' (agg_rows_common.gate_reference, with the Linear's parameters as leaves): G = sigmoid(X_h v
    + b), W = softmax_h G, out = sum_h W[:, h] X_h, and every gradient"""
    import torch
    X, v, b = leaves(X), leaf(p["v"]), leaf(p["b"])
    Z = torch.stack([x @ v + b for x in X], 1)
    G = torch.sigmoid(Z)
    W = torch.softmax(G, dim=1)
    out = sum(W[:, h:h + 1] * X[h] for h in range(len(X)))
    res = {"out": out, "W": W.detach(), "G": G.detach(), **grads([(out, p["gout"])], {"v": v, "b": b}, X, inner=Z)}
    dz = res.pop("inner").abs()
    # the Linear's gradients are sums over rows and hops of cancelling terms dZ x: the sums of the ABSOLUTE terms (truth_report's cond)
    res["cond:dv"] = sum(dz[:, h] @ X[h].detach().abs() for h in range(len(X)))
    res["cond:db"] = dz.sum().reshape(1)
    return res


def ref_recursive(X, p):
    """IterateLearnableWeightedMessageOp 'recursive': the reference's loop as written (agg_rows_common.recursive_step_by_step)"""
    import torch
    Xl, wt, b = leaves(X), leaf(p["wt"]), leaf(p["b"])
    out, W = recursive_step_by_step(Xl, wt.reshape(-1), b)
    res = {"out": out, "W": W.detach(), **grads([(out, p["gout"])], {"wt": wt, "b": b}, Xl)}
    if X[0].dtype == torch.float64:
        res.update(recursive_conditions(_np(X), {k: v.numpy() for k, v in p.items()}))
    return res


def recursive_conditions(X, p):
    """truth_report's condition magnitudes of the recursion's gradients, float64: the backward pass with every term replaced by its
    absolute value (the sums of the ABSOLUTE terms).  The backward of step i is a soft-max backward, gz_k = w_k (gw_k - sum_m gw_m
    w_m), whose difference cancels where one incoming gw dwarfs the others (a hop that holds 3e38: gw = <dOut, x> ~ 1e38) and the
    weights are nearly equal; the rounding of the weights then shows in the result at the scale of the terms, not of their
    difference, in any float32 evaluation.  On the per-row scalars a_h = <x_h, w_x>, c_h = <x_h, w_acc> (device.recursive_weights):
        step i : s_i = sigmoid(a_i + sum_{j<i} w^{i-1}_j c_j + b),  w^i = softmax(w^{i-1}_0 .. w^{i-1}_{i-1}, s_i)
        back   : Gz_k = w^i_k (Gw_k + sum_m Gw_m w^i_m),  P = Gz_i s_i (1 - s_i),  Da_i = P,  Db += P,  Dc_j += P w^{i-1}_j,
                 Gw_j <- Gz_j + P |c_j|                    (every quantity >= 0; Gw starts as sum_c |dOut| |x_h|)"""
    H = len(X)
    wx, wacc, bias = p["wt"][0], p["wt"][1], float(p["b"][0])
    with np.errstate(all="ignore"):
        a = np.stack([x @ wx for x in X], 1)
        c = np.stack([x @ wacc for x in X], 1)
        hist, sv = [np.ones((len(a), 1))], [None]
        for i in range(1, H):
            s_i = 1.0 / (1.0 + np.exp(-(a[:, i] + (hist[-1] * c[:, :i]).sum(1) + bias)))
            z = np.concatenate((hist[-1], s_i[:, None]), 1)
            e = np.exp(z - z.max(1, keepdims=True))
            hist.append(e / e.sum(1, keepdims=True))
            sv.append(s_i)
        Gw = np.stack([(np.abs(p["gout"]) * np.abs(x)).sum(1) for x in X], 1)
        Da, Dc, Db = np.zeros_like(a), np.zeros_like(a), np.zeros(len(a))
        for i in range(H - 1, 0, -1):
            w = hist[i]
            Gz = w * (Gw[:, :i + 1] + (Gw[:, :i + 1] * w).sum(1, keepdims=True))
            P = Gz[:, i] * sv[i] * (1.0 - sv[i])
            Da[:, i] = P
            Db += P
            Dc[:, :i] += P[:, None] * hist[i - 1]
            Gw = Gw.copy()
            Gw[:, :i] = Gz[:, :i] + P[:, None] * np.abs(c[:, :i])
        W = hist[-1]
        ax = [np.abs(x) for x in X]
        dwt = np.stack([sum(Da[:, h] @ ax[h] for h in range(H)), sum(Dc[:, h] @ ax[h] for h in range(H))])
        dX = np.stack([W[:, h:h + 1] * np.abs(p["gout"]) + Da[:, h:h + 1] * np.abs(wx) + Dc[:, h:h + 1] * np.abs(wacc) for h in range(H)])
    import torch
    return {"cond:dwt": torch.from_numpy(dwt), "cond:db": torch.from_numpy(Db.sum().reshape(1)), "cond:dX": torch.from_numpy(dX)}


def nafs_torch(X):
    """over_smooth_distance_op.py:11-33 in the dtype of X (oracle.nafs_weights / agg_over_smooth_distance state it in float32)"""
    import torch
    eps = torch.tensor(1e-10, dtype=torch.float32).to(X[0].dtype)
    n0 = (X[0] * X[0]).sum(1).sqrt() + eps
    W = torch.softmax(torch.stack([((X[0] * x).sum(1) / ((x * x).sum(1).sqrt() + eps)) / n0 for x in X], 1), dim=1)
    acc = torch.zeros_like(X[0])
    for h, x in enumerate(X):
        acc = acc + W[:, h:h + 1] * x
    return acc, W


def nafs_statement(X):
    """(out, W): the oracle in float32, the same expression in torch for any other dtype"""
    import torch
    if X[0].dtype == torch.float32:
        import oracle
        with np.errstate(all="ignore"):
            return _t(oracle.agg_over_smooth_distance(_np(X)), X[0]), _t(oracle.nafs_weights(_np(X)), X[0])
    return nafs_torch(X)


def ref_nafs(X, p):
    out, W = nafs_statement(X)
    return {"out": out, "W": W}


def emit_hops(H):
    return sorted({0, H // 2, H - 1})


PREFIX_DIVISOR = 3.0


def ref_prefix(combine):
    """every requested prefix X_0 .. X_h of the NAFS sweep, combined with what an earlier pass left: 0 store, 1 add, 2 add and one
    true division, 3 the NaN-propagating maximum"""
    def ref(X, p):
        import torch
        outs = []
        for h in emit_hops(len(X)):
            o = nafs_statement(X[:h + 1])[0]
            if combine in (1, 2):
                o = p["old"] + o
            if combine == 2:
                o = o / torch.tensor(PREFIX_DIVISOR, dtype=torch.float32).to(o.dtype)
            if combine == 3:
                o = torch.maximum(p["old"], o)
            outs.append(o)
        return {"out": torch.stack(outs)}
    return ref


# ---- the wrappers of sgl_amd/device.py ---------------------------------------------------------------------------------------------------
def _dev():
    from sgl_amd import _lib
    from sgl_amd import device as dev
    return _lib, dev


def gpu_reduce(kind):
    def gpu(X, p):
        _lib, dev = _dev()
        op = {"sum": _lib.SGL_REDUCE_SUM, "mean": _lib.SGL_REDUCE_MEAN, "max": _lib.SGL_REDUCE_MAX, "min": _lib.SGL_REDUCE_MIN, "wsum": _lib.SGL_REDUCE_WSUM}[kind]
        return {"out": dev.hop_reduce(op, X, p["w1"] if kind == "wsum" else None)}
    return gpu


def gpu_select(kind):
    def gpu(X, p):
        _lib, dev = _dev()
        X = leaves(X)
        out = dev.hop_reduce_grad(_lib.SGL_REDUCE_MAX if kind == "max" else _lib.SGL_REDUCE_MIN, X)
        return {"out": out, **grads([(out, p["gout"])], {}, X)}
    return gpu


def gpu_lincomb(X, p):
    import torch
    return {"out": torch.stack(_dev()[1].hop_lincomb(X, p["lin"]))}


def gpu_wsum1d(X, p):
    w = leaf(p["w1"])
    out = _dev()[1].hop_wsum1d(X, w)
    return {"out": out, **grads([(out, p["gout"])], {"w1": w})}


def gpu_wsum2d(X, p):
    X, w = leaves(X), leaf(p["w2"])
    out = _dev()[1].hop_wsum2d(X, w)
    return {"out": out, **grads([(out, p["gout"])], {"w2": w}, X)}


def gpu_scores(X, p):
    v = leaf(p["v"])
    P = _dev()[1].hop_scores(X, v)
    return {"P": P, **grads([(P, p["gw"])], {"v": v})}


def gpu_scores2(X, p):
    mask, h0, h1 = scores2_args(len(X))
    v, u = leaf(p["v"]), leaf(p["u"])
    P, A = _dev()[1].hop_scores2(X, v, u, mask, h0, h1)
    A = A[:, None]
    return {"P": P, "A": A, **grads([(P, p["gw"][:, h0:h1]), (A, p["ga"])], {"v": v, "u": u})}


def gpu_colsum(shared):
    def gpu(X, p):
        return {"out": _dev()[1].hop_colsum(X, p["ws"] if shared else p["w2"], shared=shared)}
    return gpu


def gpu_gate(X, p):
    import torch
    dev = _dev()[1]
    X, v, b = leaves(X), leaf(p["v"]), leaf(p["b"])
    out, W = dev.hop_gate(X, v, b, return_weights=True)
    res = {"out": out, "W": W.detach(), **grads([(out, p["gout"])], {"v": v, "b": b}, X)}
    if dev.gate_fusable(X):                              # the sigmoid outputs are an output of the fused kernel alone
        with torch.no_grad():
            o2, w2, res["G"] = dev._gate_launch(p["v"], p["b"], [x.detach() for x in X], True)
        res["out (inference)"], res["W (inference)"] = o2, w2
    return res


def gpu_recursive(X, p):
    X, wt, b = leaves(X), leaf(p["wt"]), leaf(p["b"])
    out, W = _dev()[1].hop_recursive(X, wt, b, return_weights=True)
    return {"out": out, "W": W.detach(), **grads([(out, p["gout"])], {"wt": wt, "b": b}, X)}


def gpu_nafs(X, p):
    out, W = _dev()[1].nafs_aggregate(X, return_weights=True)
    return {"out": out, "W": W}


def gpu_prefix(combine):
    def gpu(X, p):
        import torch
        dev = _dev()[1]
        emit = emit_hops(len(X))
        outs = None
        if combine:
            outs = [dev.alloc_rows(N, X[0].shape[1], X[0].device) for _ in emit]
            for o in outs:
                o.copy_(p["old"])
        return {"out": torch.stack(dev.nafs_prefix(X, emit, outs=outs, combine=combine, divisor=PREFIX_DIVISOR, outs_padded=bool(combine)))}
    return gpu


# the same names on both sides where the wrapper returns more than the statement states
ALIASES = {"out (inference)": "out", "W (inference)": "W"}

Family = collections.namedtuple("Family", "name ref gpu reduced kernel bf16 takes")


def _registers(s):
    return not s.dense and s.d <= 512 and s.H <= 16


FAMILIES = collections.OrderedDict((f.name, f) for f in [
    *[Family(f"reduce_{k}", ref_reduce(k), gpu_reduce(k), (), None, False, lambda s: True) for k in ("sum", "mean", "max", "min", "wsum")],
    *[Family(f"reduce_grad_{k}", ref_select(k), gpu_select(k), (), None, False, lambda s: True) for k in ("max", "min")],
    Family("lincomb", ref_lincomb, gpu_lincomb, (), None, False, lambda s: s.H <= 16),
    Family("wsum1d", ref_wsum1d, gpu_wsum1d, ("dw1",), None, False, lambda s: True),
    Family("wsum2d", ref_wsum2d, gpu_wsum2d, (), "rowdot_reg", False, lambda s: True),
    Family("scores", ref_scores, gpu_scores, ("dv",), None, False, lambda s: True),
    Family("scores2", ref_scores2, gpu_scores2, ("dv", "du"), "rowdot2", False, _registers),            # no general kernel: refused
    # (beyond 16 hops and on unaligned rows hop_colsum takes its documented torch route: held to the same rule)
    *[Family(f"colsum_{'shared' if sh else 'per_hop'}", ref_colsum(sh), gpu_colsum(sh), ("out",), None, False, lambda s: True)
      for sh in (False, True)],
    Family("gate", ref_gate, gpu_gate, ("dv", "db"), "gate", False, lambda s: True),
    Family("recursive", ref_recursive, gpu_recursive, ("dwt", "db"), "recursive", False, lambda s: True),
    Family("nafs", ref_nafs, gpu_nafs, (), "nafs", False, lambda s: True),
    *[Family(f"prefix_{c}", ref_prefix(c), gpu_prefix(c), (), "prefix", False, lambda s: not s.dense and s.d <= 512) for c in range(4)],
    *[Family(f"bf16_reduce_{k}", ref_reduce(k), gpu_reduce(k), (), None, True, lambda s: True) for k in ("sum", "mean", "max", "min", "wsum")],
    Family("bf16_nafs", ref_nafs, gpu_nafs, (), "nafs", True, lambda s: True),
])


def family_shapes(fam):
    return [s for s in shapes() if fam.takes(s) and (s != ONLY_16X3 or fam.name == "scores2")]


def cases():
    """[(family name, k, shape)]: k = the shape's position in the family's list, which picks its injections"""
    return [(name, k, s) for name, fam in FAMILIES.items() for k, s in enumerate(family_shapes(fam))]


def kernel_of(fam, s):
    """the register-resident instance the family's entry point launches for this shape (None: a general path, or no such kernel).
    Dense hops of width d % 4 != 0 are not 16-byte aligned; the dW row-dot of hop_wsum2d reads a dense gradient when d % 4 != 0"""
    if fam.kernel is None:
        return None
    return expected_kernel(fam.kernel, s.d, s.H, s.tuning, aligned=not s.dense, g_unaligned=fam.kernel == "rowdot_reg" and s.d % 4 != 0)


def tensors(hops, p, dtype):
    import torch
    return [torch.from_numpy(x).to(dtype) for x in hops], {k: torch.from_numpy(a).to(dtype) for k, a in p.items()}


def statement(fam, hops, p, dtype):
    """{name: numpy array} of the family's statement in `dtype`"""
    X, pt = tensors(hops, p, dtype)
    return {k: v.detach().numpy() for k, v in fam.ref(X, pt).items()}


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def independent(clean32, poisoned32):
    """entries whose float32 statement has the same bits on both inputs"""
    return bits(clean32) == bits(poisoned32)


def masks(a):
    return np.isnan(a), np.isposinf(a), np.isneginf(a)


def outputs(statement_):
    """a statement without its condition magnitudes ("cond:<name>")"""
    return {k: a for k, a in statement_.items() if not k.startswith("cond:")}


def row_axis(fam, name, a):
    return None if name in fam.reduced else a.ndim - 2


HUGE = 2.0 ** 64


def finite_or_zero(cond):
    return None if cond is None else np.where(np.isfinite(cond), cond, 0.0)


def apply_rule(what, s32_clean, s32, s64, got_clean, got, worst=None, cond=None):
    """the failures (a list of tuples, empty when the kernel obeys the rule) of ONE output; worst: {"ratio": ...} updated with
    err / bound of the truth_report on the touched finite entries; cond: truth_report's condition magnitudes (the float64
    statement's "cond:<name>"), for the gradients of a Linear"""
    import oracle
    bad = []
    if not (s32.shape == s64.shape == got.shape == got_clean.shape):
        return [(what, "shapes", s32.shape, got.shape)]
    ind = independent(s32_clean, s32)
    changed = ind & (bits(got_clean) != bits(got))
    if changed.any():
        bad.append((what, "independent entries changed", int(changed.sum()), tuple(int(i) for i in np.argwhere(changed)[0])))
    touched = ~ind
    for kind, ms, mg in zip(("nan", "+inf", "-inf"), masks(s32), masks(got)):
        diff = touched & (ms != mg)
        if diff.any():
            at = tuple(int(i) for i in np.argwhere(diff)[0])
            bad.append((what, f"{kind} mask", int(diff.sum()), at, float(s32[at]), float(got[at])))
    fin = touched & np.isfinite(s32) & np.isfinite(got) & np.isfinite(s64)
    # truth_report normalises by the largest entry of the truth: the entries that descend from an injected +-3e38 (about 1e37) would
    # leave the other touched entries of the row unchecked, so the two groups are reported apart.  HUGE is no tolerance: every clean
    # input and parameter is below 2^8 and an output sums at most 77 * 600 * 17 < 2^20 products of them, so nothing above 2^64 can
    # come from anywhere else.
    huge = np.abs(s64) >= HUGE
    for group, sel in (("touched finite entries", fin & ~huge), ("touched finite entries from +-3e38", fin & huge)):
        if not sel.any():
            continue
        rep = oracle.truth_report(got[sel], s32[sel], s64[sel], cond=None if cond is None else finite_or_zero(cond)[sel])
        if worst is not None:
            worst["ratio"] = max(worst.get("ratio", 0.0), rep["err_got"] / max(rep["bound"], rep["cond_bound_max"], 1e-300))
        if not rep["ok"]:
            bad.append((what, group, rep))
    return bad


def weight_rows(w, roundings=4):
    """(ok, figure): rows of soft-max weights are finite, non-negative and sum to 1 within `roundings` float32 roundings (4: the
    rule of test_gpu_agg_variants.Report.weights; None: the figure is only reported)"""
    w64 = np.asarray(w, dtype=np.float64)
    off = float(np.abs(w64.sum(1) - 1.0).max()) if np.isfinite(w64).all() else float("inf")
    return bool(np.isfinite(w64).all() and (w64 >= 0).all() and (roundings is None or off <= roundings * ROUNDING)), off / ROUNDING


# ---- the regimes: finite, ill-conditioned ----------------------------------------------------------------------------------------------
NAFS_SCALES = (-70, -50, -33, 0, 50)
DUPLICATE_ROWS = (5, 41)             # every hop equals hop 0
NEGATED_ROWS = (9, 60)               # every hop h >= 1 equals -X_0


def nafs_regime(d, H, s):
    """correlated hops X_h = (1 - 0.15 h) X_0 + 0.15 h N_h (the cosines spread out instead of sitting near 0), rows whose hops all
    equal hop 0, rows with hop h = -X_0, the zero rows of host_hops, everything scaled by 2^s (exact)"""
    base = host_hops(d, H)
    out = []
    for h in range(H):
        t = np.float32(min(0.15 * h, 1.0))
        x = ((np.float32(1.0) - t) * base[0] + t * base[h]).astype(np.float32) if h else base[0].copy()
        if h:
            x[list(DUPLICATE_ROWS)] = base[0][list(DUPLICATE_ROWS)]
            x[list(NEGATED_ROWS)] = -base[0][list(NEGATED_ROWS)]
            x[3] = 0.0
        out.append(np.ascontiguousarray(x * np.float32(2.0 ** s)))
    return out


def nafs_cosines(hops):
    """the float64 scores <X_0, X_h> / (|X_h| + 1e-10) / (|X_0| + 1e-10), [n, H]"""
    x0 = hops[0].astype(np.float64)
    eps = float(np.float32(1e-10))
    n0 = np.sqrt((x0 * x0).sum(1)) + eps
    return np.stack([(x0 * x.astype(np.float64)).sum(1) / (np.sqrt((x.astype(np.float64) ** 2).sum(1)) + eps) / n0 for x in hops], 1)


GATE_TARGETS = (20.0, -20.0, 90.0, -90.0, 200.0, -200.0)


def gate_regime(d, H):
    """(hops, p, {target: rows}): rows 10 + 6 k + j hold the pre-sigmoid score GATE_TARGETS[j] at EVERY hop, the other rows stay O(1).
    The hops are rebuilt so that <X_h[n], v> is the target exactly in float64 up to the rounding of the stored float32 values: the
    component of the row along v is replaced, X_h[n] += (target - b - <X_h[n], v>) v / |v|^2."""
    hops = [x.copy() for x in host_hops(d, H)]
    p = parameters(d, H)
    v64 = p["v"].astype(np.float64)
    rows = {t: [10 + 6 * k + j for k in range(4)] for j, t in enumerate(GATE_TARGETS)}
    for t, rr in rows.items():
        for x in hops:
            for n in rr:
                x[n] = (x[n].astype(np.float64) + (t - float(p["b"][0]) - x[n].astype(np.float64) @ v64) * v64 / (v64 @ v64)).astype(np.float32)
    return hops, p, rows


def gate_scores(hops, p):
    return np.stack([x.astype(np.float64) @ p["v"].astype(np.float64) + float(p["b"][0]) for x in hops], 1)


def recursive_regime(d, H):
    """(hops, p, {target: rows}) for the recursion: its score at step i is <X_i, w_x> + <acc, w_acc> + b with acc a convex
    combination of the hops, so a row whose hops ALL have <X_h, w_x> = target - b and <X_h, w_acc> = 0 scores the target at every
    step, whatever the weights are.  Both components are set by a least-squares correction in the plane of (w_x, w_acc)."""
    hops = [x.copy() for x in host_hops(d, H)]
    p = parameters(d, H)
    A = p["wt"].astype(np.float64)                                       # [2, d]
    pinv = A.T @ np.linalg.inv(A @ A.T)                                  # [d, 2]
    rows = {t: [10 + 6 * k + j for k in range(4)] for j, t in enumerate(GATE_TARGETS)}
    for t, rr in rows.items():
        for x in hops:
            for n in rr:
                x64 = x[n].astype(np.float64)
                x[n] = (x64 + pinv @ (np.array([t - float(p["b"][0]), 0.0]) - A @ x64)).astype(np.float32)
    return hops, p, rows


def recursive_scores(hops, p):
    """the float64 pre-sigmoid score of every step of the reference's loop, [n, H]"""
    import torch
    X, pt = tensors(hops, p, torch.float64)
    wt, acc, weights, zs = pt["wt"].reshape(-1), X[0], None, []
    for i in range(len(X)):
        z = torch.hstack((X[i], acc)) @ wt.view(-1, 1) + pt["b"]
        zs.append(z)
        score = torch.sigmoid(z)
        weights = torch.softmax(score if weights is None else torch.hstack((weights, score)), dim=1)
        acc = sum(weights[:, j:j + 1] * X[j] for j in range(i + 1))
    return torch.hstack(zs).numpy()


# ---- K16 (include/sgl_ensemble.h) with one poisoned element --------------------------------------------------------------------------------
ENSEMBLE_SHAPE = dict(n_rows=N, d=100, S=3, H=2, B=63)


def ensemble_problem(mode):
    """(X[h][s], W, idx, G) of a small K16 problem in the reference's parameter layout (ensemble_common.make_weights)"""
    e = ENSEMBLE_SHAPE
    rng = np.random.default_rng(41 + len(mode))
    X = [[rng.standard_normal((e["n_rows"], e["d"])).astype(np.float32) for _ in range(e["S"])] for _ in range(e["H"])]
    W = ec.make_weights(mode, e["S"], e["H"], e["d"], rng)
    idx = ec.make_index(e["B"], rng, n_rows=e["n_rows"])
    n_groups = ec.kernel_shape(mode, e["S"], e["H"])[0]
    G = [rng.standard_normal((e["B"], e["d"])).astype(np.float32) for _ in range(n_groups)]
    return X, W, idx, G


def ensemble_statement(mode, X, W, idx, G, dtype):
    """{"out": [groups, B, d], "dW": the parameter gradients flattened} of the aggregator of `mode`, plain torch in `dtype`, in the
    order ensemble_common states: the products summed in member order, then the division; dW = (the sum of the products X G)
    divided -- not a sum of X (G / S), which differs where X G overflows"""
    import torch
    H, S = len(X), len(X[0])
    Xt = [[torch.from_numpy(x).to(dtype)[torch.from_numpy(idx)] for x in row] for row in X]
    Gt = [torch.from_numpy(g).to(dtype) for g in G]
    div = torch.tensor(float(S), dtype=dtype)
    if mode == "fast":
        Wt = torch.from_numpy(W).to(dtype)
        outs = [sum(Xt[h][s] * Wt[s * H + h, 0] for s in range(S) for h in range(H))]
        dW = [torch.stack([(Xt[h][s] * Gt[0]).sum() for s in range(S) for h in range(H)])]
    else:
        Wt = [torch.from_numpy(w).to(dtype) for w in W]
        outs = [sum(Xt[h][s] * (Wt[h][:, s][None, :] if mode == "per_feature" else Wt[h][0, s]) for s in range(S)) / div for h in range(H)]
        if mode == "per_feature":
            dW = [(torch.stack([(Xt[h][s] * Gt[h]).sum(0) for s in range(S)], 1) / div).reshape(-1) for h in range(H)]
        else:
            dW = [torch.stack([(Xt[h][s] * Gt[h]).sum() for s in range(S)]) / div for h in range(H)]
    return {"out": torch.stack(outs).numpy(), "dW": torch.stack(dW).numpy()}


def ensemble_injections(mode):
    """one element of a matrix (a row the index takes, and one it does not take) or of a weight, every value once per place"""
    X, W, idx, G = ensemble_problem(mode)
    e = ENSEMBLE_SHAPE
    rows = [int(i) % e["n_rows"] for i in idx]
    # a row the index takes ONCE, at a column where every incoming gradient is below 1: 3e38 G then overflows in no order of the
    # sum over the rows (two terms 3e38 g of one sign, or one |g| > 1.13, overflow in one order and cancel in another)
    at = next(i for i in range(3, len(rows)) if rows.count(rows[i]) == 1)
    taken = rows[at]
    calm = [c for c in (0, e["d"] - 1, e["d"] // 2, *range(1, e["d"] - 1)) if all(abs(float(g[at, c])) < 1.0 for g in G)][:3]
    free = next(r for r in range(e["n_rows"]) if r not in set(rows))
    out = []
    for k, (name, value) in enumerate(VALUES):
        out.append(("matrix", (k % e["H"], k % e["S"], taken, calm[k % 3]), name, value))
        out.append(("matrix", (k % e["H"], (k + 1) % e["S"], free, e["d"] // 2), name, value))
        out.append(("weight", (k % e["H"], k % e["S"], (0, e["d"] - 1, e["d"] // 2)[k % 3]), name, value))
    return out


def ensemble_poisoned(mode, X, W, inj):
    """(X, W) with the injected element replaced; a weight of `shared` / `fast` has no column"""
    kind, at, _, value = inj
    H, S = len(X), len(X[0])
    if kind == "matrix":
        h, s, r, c = at
        X = [list(row) for row in X]
        X[h][s] = X[h][s].copy()
        X[h][s][r, c] = value
        return X, W
    h, s, c = at
    if mode == "fast":
        W = W.copy()
        W[s * H + h, 0] = value
    else:
        W = [w.copy() for w in W]
        W[h][c if mode == "per_feature" else 0, s] = value
    return X, W

"""Every compiled instance of the row-register aggregator kernels of csrc/sgl_aggregate.hip, launched and checked on a real
MI355X: run with `-m gpu`.

hop_rowdot_reg_kernel (the dW of hop_wsum2d), nafs_fused_kernel, gate_fused_kernel, recursive_fused_kernel, hop_rowdot2_reg_kernel
and nafs_prefix_kernel keep the hop rows of a node in registers and are compiled per lane layout (LPR lanes x CH chunks per row)
and hop capacity HMAX.  Which instance an entry point launches is decided by sgl::row_instance (csrc/sgl_core.cpp) from
the width, the hop count and three tuning keys; that rule is restated in agg_rows_common.expected_kernel, and every launch made
here is checked against the name of the kernel that really ran, as the profiler reports it (Trace).  Each family's test ends with
"the instances seen are exactly the compiled ones".

Inputs are hostile where the kernels promise not to look: the pad columns d .. pitch of every hop buffer (and of a padded dOut)
hold NaN in one run and 1e30 in another, the outputs are pre-filled with a sentinel.  Values are compared with a float64
statement of the operation (the truth) through oracle.truth_report -- at most twice as far from the truth as the same statement
in float32 -- and, for NAFS, with the oracle under the project's parity contract.  No tolerance is chosen in this file."""
import numpy as np
import pytest
import torch

import oracle
from agg_rows_common import (BIAS, FAMILIES, HOP_SWEEP, N_ROWS, WIDTH_8X5, case_list, compiled_variants, expected_kernel, gate_reference,
                             parse_agg_kernel_name, recursive_step_by_step, t32, t64, tuned, vector)
from inputs import hash_matrix
from sgl_amd import _lib
from sgl_amd import device as dev

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
POISONS = (float("nan"), 1e30)
ROUNDING = 2.0 ** -24               # one float32 rounding of a value near 1 (the unit of oracle.TRUTH_FLOOR)
NAN = float("nan")


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


# ---- which kernels ran --------------------------------------------------------------------------------------------------------
class Trace:
    """Runs launches under torch.profiler and checks, at exit, that the kernels of the six families that really ran are, in
    order, the ones `expect()` announced (None = "no fused kernel": nothing of the families may run); everything else is ignored.
    seen[family] collects the template arguments.  A profiler that reports no kernel names fails the comparison."""

    def __init__(self):
        self.expected, self.seen = [], {f: set() for f in FAMILIES}

    def expect(self, label, kernel):
        if kernel is not None:
            self.expected.append((label, kernel))

    def __enter__(self):
        from torch.profiler import ProfilerActivity, profile
        self.prof = profile(activities=[ProfilerActivity.CUDA])            # kernel names are all that is read
        self.prof.__enter__()
        return self

    def __exit__(self, et, ev, tb):
        torch.cuda.synchronize()
        self.prof.__exit__(et, ev, tb)
        if et is not None:
            return False
        from torch.autograd import DeviceType
        evs = sorted((e for e in self.prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
        got = [p for p in (parse_agg_kernel_name(e.name) for e in evs) if p is not None]
        assert len(got) == len(self.expected), (len(got), len(self.expected), len(evs), got[:3], self.expected[:3])
        wrong = [(i, lab, g, w) for i, (g, (lab, w)) in enumerate(zip(got, self.expected)) if g != w]
        assert not wrong, (len(wrong), wrong[:8])
        for fam, args in got:
            self.seen[fam].add(args)
        return False


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
_HOST = {}


def host_hops(n, d, n_hops):
    """hop h = hash_matrix scaled by (1 - 0.04 h); row 1 of hop 0 is zero (cosine 0 with every hop) and row 3 of every hop"""
    key = (n, d)
    have = _HOST.setdefault(key, [])
    for h in range(len(have), n_hops):
        x = np.ascontiguousarray((hash_matrix(n, d, seed=31 * d + h) * np.float32(1.0 - 0.04 * h)).astype(np.float32))
        if n > 2 and h == 0:
            x[1] = 0.0
        if n > 4:
            x[3] = 0.0
        have.append(x)
    return have[:n_hops]


def poisoned_rows(x, cuda, poison):
    """x in a dev.alloc_rows buffer whose pad columns d .. pitch hold `poison` (inside the row's own pitch: never out of bounds)"""
    n, d = x.shape
    t = dev.alloc_rows(n, d, cuda, zero_pad=False)
    dev.padded_parent(t).fill_(poison)
    t.copy_(torch.from_numpy(x))
    return t


_DEV = {}


def device_hops(n, d, n_hops, cuda):
    """{poison: [hop tensors]}: uploaded once per (n, d), longer lists extend shorter ones"""
    host = host_hops(n, d, n_hops)
    per = _DEV.setdefault((n, d), {p_: [] for p_ in range(len(POISONS))})
    for k, poison in enumerate(POISONS):
        for h in range(len(per[k]), n_hops):
            per[k].append(poisoned_rows(host[h], cuda, poison))
    if len(_DEV) > 12:
        _DEV.pop(next(iter(_DEV)))
    return [per[k][:n_hops] for k in range(len(POISONS))]


def padded_out(n, d, cuda):
    """(view, parent, pad): an alloc_rows output pre-filled with the sentinel, pad columns included"""
    t = dev.alloc_rows(n, d, cuda, zero_pad=False)
    parent = dev.padded_parent(t)
    parent.fill_(SENTINEL)
    return t, parent, dev.own_pad(t)


def sliced_out(n, d, cuda, rows_extra=3):
    """(view, wide): columns 4 .. 4 + d of the first n rows of a wider, longer matrix full of the sentinel; 16-byte aligned"""
    wide = torch.full((n + rows_extra, dev.round_up(d, 4) + 8), SENTINEL, dtype=torch.float32, device=cuda)
    return wide[:n, 4:4 + d], wide


def untouched_outside(view, wide, c0=4):
    """everything of `wide` outside the view still holds the sentinel"""
    n, d = view.shape
    w = wide.clone()
    w[:n, c0:c0 + d] = SENTINEL
    return bool((w == SENTINEL).all())


def small_out(n, k, cuda):
    """(view, wide): an [n, k] score / weight matrix as columns 2 .. 2 + k of a longer, wider sentinel matrix"""
    wide = torch.full((n + 3, k + 5), SENTINEL, dtype=torch.float32, device=cuda)
    return wide[:n, 2:2 + k], wide


def ld(t):
    return t.stride(0)


def call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()), name)


class Report:
    """collects failed checks (so that one run shows all of them) and the largest figures for the printed summary"""

    def __init__(self, family):
        self.family, self.bad, self.worst, self.cases = family, [], {}, 0

    def truth(self, label, what, got, ref32, ref64, cond=None):
        got = got.detach().cpu().numpy()
        if not np.isfinite(got).all():
            self.bad.append((label, what, "not finite"))
            return
        rep = oracle.truth_report(got, ref32.numpy(), ref64.numpy(), cond=None if cond is None else cond.numpy())
        w = self.worst.setdefault(what, {"err_got": 0.0, "err_ref": 0.0, "ratio": 0.0})
        w["err_got"], w["err_ref"] = max(w["err_got"], rep["err_got"]), max(w["err_ref"], rep["err_ref"])
        w["ratio"] = max(w["ratio"], rep["err_got"] / max(rep["bound"], 1e-300))
        if not rep["ok"]:
            self.bad.append((label, what, rep))

    def check(self, ok, label, what):
        if not ok:
            self.bad.append((label, what))

    def weights(self, label, w):
        """rows of soft-max weights: non-negative, summing to 1 within 4 float32 roundings"""
        w64 = w.detach().cpu().double()
        off = float((w64.sum(1) - 1.0).abs().max())
        self.worst["weight row sum - 1 (roundings)"] = max(self.worst.get("weight row sum - 1 (roundings)", 0.0), off / ROUNDING)
        self.check(bool((w64 >= 0).all()) and off <= 4 * ROUNDING, label, ("weight rows", off / ROUNDING))

    def finish(self, seen):
        print(f"\n[{self.family}] {self.cases} cases, {len(seen)} of {len(compiled_variants(self.family))} instances seen; worst: {self.worst}")
        assert not self.bad, (len(self.bad), self.bad[:10])
        assert seen == compiled_variants(self.family), sorted(compiled_variants(self.family) - seen)


def same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


def sweep(family, cuda, one_case, **kw):
    """every case of the family's list under one Trace; the layout keys are set per case"""
    rep = Report(family)
    with Trace() as tr:
        for n, d, n_hops, tuning in case_list(family):
            with tuned(**tuning):
                one_case(tr, rep, cuda, n, d, n_hops, tuning, **kw)
            rep.cases += 1
    rep.finish(tr.seen[family])
    assert all(not v for f, v in tr.seen.items() if f != family)


# ---- the gate --------------------------------------------------------------------------------------------------------------------
def gate_case(tr, rep, cuda, n, d, H, tuning):
    label = ("gate", n, d, H, tuple(tuning.items()))
    kern = expected_kernel("gate", d, H, tuning)
    host = host_hops(n, d, H)
    by_poison = device_hops(n, d, H, cuda)
    v = vector(d, 7 * d + 1, 0.3)
    vp = dev._padded_vec(torch.from_numpy(v), d, cuda, tail=torch.tensor([BIAS]))      # [v | 0-pad | bias]

    def padded(feats, bias):
        out, parent, pad = padded_out(n, d, cuda)
        w, ww = small_out(n, H, cuda)
        g, gw = small_out(n, H, cuda)
        ptrs, lds = _lib.hop_arrays(feats)
        tr.expect(label, kern)
        call("sgl_hop_gate_padded_f32", H, ptrs, lds, _lib.ptr(vp), bias, _lib.ptr(out), ld(out), pad, _lib.ptr(w), ld(w), _lib.ptr(g),
             ld(g), n, d)
        return out, parent, pad, (w, ww), (g, gw)

    out, parent, pad, (w, ww), (g, gw) = padded(by_poison[0], NAN)              # the bias read from the device
    y64, w64, g64 = gate_reference(host, v, torch.float64)
    y32, w32, g32 = gate_reference(host, v, torch.float32)
    rep.truth(label, "out", out, y32, y64)
    rep.truth(label, "W", w, w32, w64)
    rep.truth(label, "G", g, g32, g64)
    rep.weights(label, w)
    rep.check(bool((parent[:, d:] == (0.0 if pad else SENTINEL)).all()), label, "pad columns of the padded output")
    rep.check(untouched_outside(w, ww, 2) and untouched_outside(g, gw, 2), label, "W / G outside their n x H")
    again = padded(by_poison[0], NAN)
    rep.check(same(again[0], out) and same(again[3][0], w) and same(again[4][0], g), label, "repeated call")
    other = padded(by_poison[1], BIAS)                                            # 1e30 pads, the bias as a host float
    rep.check(same(other[0], out) and same(other[3][0], w) and same(other[4][0], g), label, "1e30 pads / host bias")
    # un-suffixed entry (pad 0) into a column slice of a wider, longer matrix
    view, wide = sliced_out(n, d, cuda)
    ptrs, lds = _lib.hop_arrays(by_poison[0])
    tr.expect(label, kern)
    call("sgl_hop_gate_f32", H, ptrs, lds, _lib.ptr(vp), BIAS, _lib.ptr(view), ld(view), None, 0, None, 0, n, d)
    rep.check(same(view, out), label, "un-suffixed entry: bits")
    rep.check(untouched_outside(view, wide), label, "un-suffixed entry: outside its columns / rows")
    with tuned(**dict(tuning, row_whole_lines=0)):
        part = padded(by_poison[0], NAN)
    rep.check(same(part[0], out), label, "row_whole_lines = 0")


def test_gate_every_instance(cuda):
    sweep("gate", cuda, gate_case)


# ---- the recursive gate --------------------------------------------------------------------------------------------------------
def recursive_case(tr, rep, cuda, n, d, H, tuning):
    label = ("recursive", n, d, H, tuple(tuning.items()))
    kern = expected_kernel("recursive", d, H, tuning)
    host = host_hops(n, d, H)
    by_poison = device_hops(n, d, H, cuda)
    wt = vector(2 * d, 11 * d + 3, 0.5 / d ** 0.5)
    dp = dev.round_up(d, 4)
    vp = torch.zeros(2 * dp + 4, dtype=torch.float32)
    vp[:d], vp[dp:dp + d], vp[2 * dp] = torch.from_numpy(wt[:d]), torch.from_numpy(wt[d:]), BIAS
    vp = vp.to(cuda)

    def launch(feats, bias, out, pad):
        mats = [small_out(n, H, cuda) for _ in range(3)]
        ptrs, lds = _lib.hop_arrays(feats)
        tr.expect(label, kern)
        call("sgl_hop_recursive_f32", H, ptrs, lds, _lib.ptr(vp), bias, _lib.ptr(out), ld(out), pad, _lib.ptr(mats[0][0]), ld(mats[0][0]),
             _lib.ptr(mats[1][0]), ld(mats[1][0]), _lib.ptr(mats[2][0]), ld(mats[2][0]), n, d)
        return mats

    out, parent, pad = padded_out(n, d, cuda)
    (w, ww), (a, aw), (c, cw) = launch(by_poison[0], NAN, out, pad)
    ref = {}
    for dt in (torch.float64, torch.float32):
        ff = [torch.from_numpy(x).to(dt) for x in host]
        wv = torch.from_numpy(wt).to(dt)
        y, wr = recursive_step_by_step(ff, wv, torch.tensor([BIAS], dtype=torch.float32).to(dt))
        ref[dt] = (y, wr, torch.stack([f @ wv[:d] for f in ff], 1), torch.stack([f @ wv[d:] for f in ff], 1))
    conds = [torch.stack([torch.from_numpy(np.abs(x)).double() @ torch.from_numpy(np.abs(part)).double() for x in host], 1)
             for part in (wt[:d], wt[d:])]
    r64, r32 = ref[torch.float64], ref[torch.float32]
    rep.truth(label, "out", out, r32[0], r64[0])
    rep.truth(label, "W", w, r32[1], r64[1])
    rep.truth(label, "A", a, r32[2], r64[2], cond=conds[0])
    rep.truth(label, "C", c, r32[3], r64[3], cond=conds[1])
    rep.weights(label, w)
    rep.check(bool((parent[:, d:] == (0.0 if pad else SENTINEL)).all()), label, "pad columns of the padded output")
    rep.check(all(untouched_outside(m, mw, 2) for m, mw in ((w, ww), (a, aw), (c, cw))), label, "W / A / C outside their n x H")
    out2, _, _ = padded_out(n, d, cuda)
    m2 = launch(by_poison[0], NAN, out2, pad)
    rep.check(same(out2, out) and all(same(x[0], y_) for x, y_ in zip(m2, (w, a, c))), label, "repeated call")
    out3, _, _ = padded_out(n, d, cuda)
    m3 = launch(by_poison[1], BIAS, out3, pad)
    rep.check(same(out3, out) and all(same(x[0], y_) for x, y_ in zip(m3, (w, a, c))), label, "1e30 pads / host bias")
    view, wide = sliced_out(n, d, cuda)
    launch(by_poison[0], BIAS, view, 0)
    rep.check(same(view, out), label, "pad 0: bits")
    rep.check(untouched_outside(view, wide), label, "pad 0: outside its columns / rows")
    out4, _, _ = padded_out(n, d, cuda)
    with tuned(**dict(tuning, row_whole_lines=0)):
        launch(by_poison[0], NAN, out4, pad)
    rep.check(same(out4, out), label, "row_whole_lines = 0")


def test_recursive_every_instance(cuda):
    sweep("recursive", cuda, recursive_case)


# ---- NAFS ------------------------------------------------------------------------------------------------------------------------
def nafs_case(tr, rep, cuda, n, d, H, tuning):
    label = ("nafs", n, d, H, tuple(tuning.items()))
    kern = expected_kernel("nafs", d, H, tuning)
    host = host_hops(n, d, H)
    by_poison = device_hops(n, d, H, cuda)

    def padded(feats):
        out, parent, pad = padded_out(n, d, cuda)
        w, ww = small_out(n, H, cuda)
        ptrs, lds = _lib.hop_arrays(feats)
        tr.expect(label, kern)
        call("sgl_nafs_padded_f32", H, ptrs, lds, _lib.ptr(out), ld(out), pad, _lib.ptr(w), ld(w), n, d)
        return out, parent, pad, w, ww

    out, parent, pad, w, ww = padded(by_poison[0])
    got, gw = out.cpu().numpy(), w.cpu().numpy()
    rep.check(bool(np.isfinite(got).all() and np.isfinite(gw).all()), label, "finite")
    rep.check(bool(np.allclose(gw, oracle.nafs_weights(host), rtol=5e-5, atol=5e-6)), label, "weights against the oracle")
    rep.check(oracle.parity_ok(got, oracle.agg_over_smooth_distance(host), 2e-5, rowwise=False), label, "output against the oracle")
    rep.weights(label, w)
    rep.check(bool((parent[:, d:] == (0.0 if pad else SENTINEL)).all()), label, "pad columns of the padded output")
    rep.check(untouched_outside(w, ww, 2), label, "W outside its n x H")
    again = padded(by_poison[0])
    rep.check(same(again[0], out) and same(again[3], w), label, "repeated call")
    other = padded(by_poison[1])
    rep.check(same(other[0], out) and same(other[3], w), label, "1e30 pads")
    view, wide = sliced_out(n, d, cuda)
    w2, _ = small_out(n, H, cuda)
    ptrs, lds = _lib.hop_arrays(by_poison[0])
    tr.expect(label, kern)
    call("sgl_nafs_f32", H, ptrs, lds, _lib.ptr(view), ld(view), _lib.ptr(w2), ld(w2), n, d)
    rep.check(same(view, out) and same(w2, w), label, "un-suffixed entry: bits")
    rep.check(untouched_outside(view, wide), label, "un-suffixed entry: outside its columns / rows")
    with tuned(**dict(tuning, row_whole_lines=0)):
        part = padded(by_poison[0])
    rep.check(same(part[0], out), label, "row_whole_lines = 0")


def test_nafs_every_instance(cuda):
    sweep("nafs", cuda, nafs_case)


# ---- dW of the per-row weighted sum ------------------------------------------------------------------------------------------------
def dout_matrices(n, d, gu, cuda):
    """(host dOut, [device dOut per poison]).  gu: rows that are only dword-aligned -- a dense [n, d] tensor when d % 4 != 0, else
    columns 1 .. 1 + d of a dense [n, d + 4] one; otherwise an alloc_rows buffer with poisoned pad columns"""
    g = np.ascontiguousarray(hash_matrix(n, d, seed=5 * d + 2))
    if not gu:
        return g, [poisoned_rows(g, cuda, p_) for p_ in POISONS]
    if d % 4:
        t = torch.from_numpy(g).to(cuda)
    else:
        t = torch.full((n, d + 4), POISONS[1], dtype=torch.float32, device=cuda)[:, 1:1 + d]
        t.copy_(torch.from_numpy(g))
    assert t.data_ptr() % 4 == 0 and (t.data_ptr() % 16 != 0 or ld(t) % 4 != 0 or n == 1)
    return g, [t, t]


def rowdot_case(tr, rep, cuda, n, d, H, tuning, gu):
    label = ("rowdot_reg", gu, n, d, H, tuple(tuning.items()))
    host = host_hops(n, d, H)
    by_poison = device_hops(n, d, H, cuda)
    g, g_dev = dout_matrices(n, d, gu, cuda)
    lddo = [ld(t) for t in g_dev]
    assert (g_dev[0].data_ptr() % 16 != 0 or lddo[0] % 4 != 0) == gu
    kern = expected_kernel("rowdot_reg", d, H, tuning, g_unaligned=gu)

    def launch(k, dw):
        ptrs, lds = _lib.hop_arrays(by_poison[k])
        tr.expect(label, kern)
        call("sgl_hop_wsum2d_bwd_f32", H, ptrs, lds, None, 0, _lib.ptr(g_dev[k]), lddo[k], _lib.ptr(dw), ld(dw), None, None, n, d)

    dw, wide = small_out(n, H, cuda)
    launch(0, dw)
    g64 = t64(g)
    truth = torch.stack([(g64 * t64(x)).sum(1) for x in host], 1)
    ref32 = torch.stack([(t32(g) * t32(x)).sum(1) for x in host], 1)
    cond = torch.stack([(g64.abs() * t64(x).abs()).sum(1) for x in host], 1)
    rep.truth(label, "dW", dw, ref32, truth, cond=cond)
    rep.check(untouched_outside(dw, wide, 2), label, "dW outside its n x H")
    dw2 = torch.full((n, H), SENTINEL, dtype=torch.float32, device=cuda)
    launch(0, dw2)
    rep.check(same(dw2, dw), label, "repeated call")
    dw3 = torch.full((n, H), SENTINEL, dtype=torch.float32, device=cuda)
    launch(1, dw3)
    rep.check(same(dw3, dw), label, "1e30 pads")


@pytest.mark.parametrize("gu", [False, True])
def test_rowdot_reg_every_instance(cuda, gu):
    rep = Report("rowdot_reg")
    with Trace() as tr:
        for n, d, n_hops, tuning in case_list("rowdot_reg"):
            with tuned(**tuning):
                rowdot_case(tr, rep, cuda, n, d, n_hops, tuning, gu)
            rep.cases += 1
    seen = tr.seen["rowdot_reg"]
    want = {v for v in compiled_variants("rowdot_reg") if v[3] == int(gu)}
    print(f"\n[rowdot_reg GU={int(gu)}] {rep.cases} cases, {len(seen)} of {len(want)} instances seen; worst: {rep.worst}")
    assert not rep.bad, (len(rep.bad), rep.bad[:10])
    assert seen == want, sorted(want - seen)


# ---- the two-part scores ---------------------------------------------------------------------------------------------------------
def rowdot2_case(tr, rep, cuda, n, d, H, tuning):
    label = ("rowdot2", n, d, H, tuple(tuning.items()))
    kern = expected_kernel("rowdot2", d, H, tuning)
    host = host_hops(n, d, H)
    by_poison = device_hops(n, d, H, cuda)
    v = vector(d, 13 * d + 5, 0.3)
    u = np.ascontiguousarray(hash_matrix(H, d, seed=17 * d + H) * np.float32(0.3))
    mask = (0xB6DB & ((1 << H) - 1)) | (1 << (H - 1))                 # two of every three hops, and the last one
    h0, h1 = (1 if H >= 3 else 0), H
    vp = dev._padded_vec(torch.from_numpy(v), d, cuda)
    ldu = dev.round_up(d, 4)
    up = torch.zeros((H, ldu), dtype=torch.float32, device=cuda)
    up[:, :d] = torch.from_numpy(u)

    def launch(k):
        p, pw = small_out(n, h1 - h0, cuda)
        a = torch.full((n + 3,), SENTINEL, dtype=torch.float32, device=cuda)
        ptrs, lds = _lib.hop_arrays(by_poison[k])
        tr.expect(label, kern)
        call("sgl_hop_rowdot2_f32", H, ptrs, lds, _lib.ptr(up), ldu, mask, _lib.ptr(vp), h0, h1, _lib.ptr(p), ld(p), _lib.ptr(a), n, d)
        return p, pw, a

    p, pw, a = launch(0)
    ref_hops = [j for j in range(H) if (mask >> j) & 1]
    for what, got, terms in (("P", p, [[(host[h], v)] for h in range(h0, h1)]), ("A", a[:n, None], [[(host[j], u[j]) for j in ref_hops]])):
        truth = torch.stack([sum(t64(x) @ t64(y_) for x, y_ in col) for col in terms], 1)
        ref32 = torch.stack([sum(t32(x) @ t32(y_) for x, y_ in col) for col in terms], 1)
        cond = torch.stack([sum(t64(x).abs() @ t64(y_).abs() for x, y_ in col) for col in terms], 1)
        rep.truth(label, what, got, ref32, truth, cond=cond)
    rep.check(untouched_outside(p, pw, 2) and bool((a[n:] == SENTINEL).all()), label, "P / A outside their rows and columns")
    again = launch(0)
    rep.check(same(again[0], p) and same(again[2], a), label, "repeated call")
    other = launch(1)
    rep.check(same(other[0], p) and same(other[2], a), label, "1e30 pads")


def test_rowdot2_every_instance(cuda):
    sweep("rowdot2", cuda, rowdot2_case)


# ---- every NAFS prefix in one pass -----------------------------------------------------------------------------------------------
def prefix_case(tr, rep, cuda, n, d, H, tuning):
    label = ("prefix", n, d, H, tuple(tuning.items()))
    kern = expected_kernel("prefix", d, H, tuning)
    host = host_hops(n, d, H)
    by_poison = device_hops(n, d, H, cuda)
    emit = sorted({0, H // 2, H - 1})                                   # hop 0, one in the middle, the last
    mask = sum(1 << h for h in emit)
    want = [oracle.agg_over_smooth_distance(host[:h + 1]) for h in emit]

    def launch(k, outs, pad, combine=0, divisor=1.0):
        ptrs, lds = _lib.hop_arrays(by_poison[k])
        optrs, olds = _lib.hop_arrays(outs)
        tr.expect(label, kern)
        call("sgl_nafs_prefix_f32", H, ptrs, lds, mask, optrs, olds, pad, combine, divisor, n, d)

    made = [padded_out(n, d, cuda) for _ in emit]
    pad = made[0][2]
    launch(0, [m[0] for m in made], pad)
    stored = [m[0] for m in made]
    for h, o, ref, m in zip(emit, stored, want, made):
        got = o.cpu().numpy()
        rep.check(bool(np.isfinite(got).all()), label, ("finite", h))
        rep.check(oracle.parity_ok(got, ref, 2e-5, rowwise=False), label, ("prefix against the oracle", h))
        rep.check(bool((m[1][:, d:] == (0.0 if pad else SENTINEL)).all()), label, ("pad columns of the padded output", h))
    for k, what, whole in ((0, "repeated call", 1), (1, "1e30 pads", 1), (0, "row_whole_lines = 0", 0)):
        more = [padded_out(n, d, cuda) for _ in emit]
        with tuned(**dict(tuning, row_whole_lines=whole)):
            launch(k, [m[0] for m in more], pad)
        rep.check(all(same(m[0], o) for m, o in zip(more, stored)), label, what)
    slices = [sliced_out(n, d, cuda) for _ in emit]
    launch(0, [s[0] for s in slices], 0)
    rep.check(all(same(s[0], o) for s, o in zip(slices, stored)), label, "pad 0: bits")
    rep.check(all(untouched_outside(*s) for s in slices), label, "pad 0: outside its columns / rows")
    # the ensemble combinations with what an earlier pass left: float32 add / add and divide / NaN-propagating max of the stored prefix
    old = np.ascontiguousarray(hash_matrix(n, d, seed=3 * d + 9))
    if n > 2:
        old[2, 0] = np.nan
    old_dev = torch.from_numpy(old).to(cuda)
    for combine, divisor, fn in ((1, 1.0, lambda o: old + o), (2, 3.0, lambda o: (old + o) / np.float32(3.0)), (3, 1.0, lambda o: np.maximum(old, o))):
        slices = [sliced_out(n, d, cuda) for _ in emit]
        for s in slices:
            s[0].copy_(old_dev)
        launch(0, [s[0] for s in slices], 0, combine, divisor)
        ok = all(np.array_equal(s[0].cpu().numpy(), fn(o.cpu().numpy()).astype(np.float32), equal_nan=True) for s, o in zip(slices, stored))
        rep.check(ok, label, ("combine", combine))
        rep.check(all(untouched_outside(*s) for s in slices), label, ("combine: outside its columns / rows", combine))


def test_prefix_every_instance(cuda):
    sweep("prefix", cuda, prefix_case)


# ---- where the fused kernels end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", [(100, 17), (513, 4)])
def test_general_path_beyond_sixteen_hops_or_512_columns(cuda, d, H):
    """one hop or one column too many: announced as "no fused kernel", so nothing of the six families may run, and the values of
    the routes behind the same calls are still right"""
    n = N_ROWS
    rep = Report("general")
    host = host_hops(n, d, H)
    feats = device_hops(n, d, H, cuda)[0]
    v = vector(d, 7 * d + 1, 0.3)
    wt = vector(2 * d, 11 * d + 3, 0.5 / d ** 0.5)
    b = torch.tensor([BIAS], device=cuda)
    for fam in ("gate", "recursive", "nafs", "rowdot_reg", "rowdot2"):
        assert expected_kernel(fam, d, H) is None
    assert not dev.gate_fusable(feats)
    with Trace() as tr:
        label = ("general", d, H)
        tr.expect(label, None)
        y, w = dev.hop_gate(feats, torch.from_numpy(v).to(cuda), b, return_weights=True)
        y64, w64, _ = gate_reference(host, v, torch.float64)
        y32, w32, _ = gate_reference(host, v, torch.float32)
        rep.truth(label, "gate out", y, y32, y64)
        rep.truth(label, "gate W", w, w32, w64)
        y, w = dev.hop_recursive(feats, torch.from_numpy(wt).to(cuda), b, return_weights=True)
        ref = {}
        for dt in (torch.float64, torch.float32):
            ref[dt] = recursive_step_by_step([torch.from_numpy(x).to(dt) for x in host], torch.from_numpy(wt).to(dt),
                                              torch.tensor([BIAS], dtype=torch.float32).to(dt))
        rep.truth(label, "recursive out", y, ref[torch.float32][0], ref[torch.float64][0])
        rep.truth(label, "recursive W", w, ref[torch.float32][1], ref[torch.float64][1])
        y, w = dev.nafs_aggregate(feats, return_weights=True)
        rep.check(bool(np.allclose(w.cpu().numpy(), oracle.nafs_weights(host), rtol=5e-5, atol=5e-6)), label, "nafs weights")
        rep.check(oracle.parity_ok(y.cpu().numpy(), oracle.agg_over_smooth_distance(host), 2e-5, rowwise=False), label, "nafs output")
        g, g_dev = dout_matrices(n, d, False, cuda)
        dw = torch.full((n, H), SENTINEL, dtype=torch.float32, device=cuda)
        ptrs, lds = _lib.hop_arrays(feats)
        call("sgl_hop_wsum2d_bwd_f32", H, ptrs, lds, None, 0, _lib.ptr(g_dev[0]), ld(g_dev[0]), _lib.ptr(dw), H, None, None, n, d)
        g64 = t64(g)
        rep.truth(label, "dW", dw, torch.stack([(t32(g) * t32(x)).sum(1) for x in host], 1), torch.stack([(g64 * t64(x)).sum(1) for x in host], 1),
                  cond=torch.stack([(g64.abs() * t64(x).abs()).sum(1) for x in host], 1))
        with pytest.raises(_lib.SglHipError):               # the two-part scores have no general kernel: refused, nothing launched
            dev.hop_scores2(feats, torch.from_numpy(v).to(cuda), torch.zeros((H, d), device=cuda), 1, 0, H)
    assert not rep.bad, rep.bad
    assert all(not s for s in tr.seen.values())
    if d > 512:
        with pytest.raises(_lib.SglHipError):
            dev.nafs_prefix(feats, [0, H - 1])


# ---- the Python wrappers take the same route -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,d,tuning", HOP_SWEEP + (((8, 5), WIDTH_8X5, {}),), ids=lambda v: str(v).replace(" ", ""))
def test_wrappers_launch_the_fused_kernels(cuda, layout, d, tuning):
    """dev.hop_gate, dev.hop_recursive, dev.nafs_aggregate, dev.hop_scores2 and the backward of dev.hop_wsum2d launch the instance
    the C entry points do: a predicate that sent them down the two-pass routes instead would leave their values right"""
    n, H = N_ROWS, 5
    host = host_hops(n, d, H)
    feats = device_hops(n, d, H, cuda)[0]
    v = torch.from_numpy(vector(d, 7 * d + 1, 0.3)).to(cuda)
    wt = torch.from_numpy(vector(2 * d, 11 * d + 3, 0.5 / d ** 0.5)).to(cuda)
    u = torch.from_numpy(np.ascontiguousarray(hash_matrix(H, d, seed=17 * d + H) * np.float32(0.3))).to(cuda)
    b = torch.tensor([BIAS], device=cuda)
    gout = torch.from_numpy(hash_matrix(n, d, seed=5 * d + 2)).to(cuda)
    wide = layout if layout != (8, 5) else (16, 3)                        # 8 x 5 is the two-part scores' alone
    with tuned(**tuning), Trace() as tr:
        for fam in ("gate", "recursive", "nafs"):
            assert expected_kernel(fam, d, H, tuning)[1][:2] == wide
        assert expected_kernel("rowdot2", d, H, tuning)[1][:2] == ((8, 5) if 129 <= d <= 160 else layout)
        assert dev.gate_fusable(feats)
        with torch.no_grad():
            tr.expect("hop_gate", expected_kernel("gate", d, H, tuning))
            yg = dev.hop_gate(feats, v, b)
            tr.expect("hop_recursive", expected_kernel("recursive", d, H, tuning))
            yr = dev.hop_recursive(feats, wt, b)
            tr.expect("nafs_aggregate", expected_kernel("nafs", d, H, tuning))
            yn = dev.nafs_aggregate(feats)
            tr.expect("hop_scores2", expected_kernel("rowdot2", d, H, tuning))
            p, a = dev.hop_scores2(feats, v, u, 0b10011, 1, H)
        w = torch.softmax(torch.from_numpy(hash_matrix(n, H, seed=d)).to(cuda), dim=1).requires_grad_(True)
        y = dev.hop_wsum2d(feats, w)
        tr.expect("hop_wsum2d backward", expected_kernel("rowdot_reg", d, H, tuning, g_unaligned=d % 4 != 0))
        y.backward(gout)
    assert all(bool(torch.isfinite(t).all()) for t in (yg, yr, yn, p, a, w.grad))
    g64 = t64(gout.cpu().numpy())
    rep = oracle.truth_report(w.grad.cpu().numpy(), torch.stack([(t32(gout.cpu().numpy()) * t32(x)).sum(1) for x in host], 1).numpy(),
                              torch.stack([(g64 * t64(x)).sum(1) for x in host], 1).numpy(),
                              cond=torch.stack([(g64.abs() * t64(x).abs()).sum(1) for x in host], 1).numpy())
    assert rep["ok"], rep
